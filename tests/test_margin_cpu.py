"""tests/margin_model.py held to independent arithmetic, and the probe held to the oracle alone, before tests/test_gpu_margins.py uses either.

The bar of an fp64 classification multiplier, 2^-51 ABSOLUTE, to first order for m = -y (1 - 1 / (1 + t)), t = exp(-y a): exp within 1 ulp moves m by
at most t / (1 + t)^2 <= 1/4 of 2^-52; the addition and the division each round a value <= 1 (2^-53 each); the final subtraction rounds a value <= 1
(2^-53).  1.75 x 2^-52 in all; 2^-51 leaves room for the second-order terms.  Measured here: 0.37 of the bar for the oracle (glibc's exp) and for the
model of the reassociated kernel's multiplier."""
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from tests import margin_model as mm

from tests.margin_cases import HI, LO, REG_LABELS, label_sets, oracle_probe, plain_update, probe_margins, reg_predictions, reg_probe

LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------------ the grid
def test_the_grid_is_fixed_and_holds_its_landmarks():
    m = mm.MARGINS
    assert m.dtype == np.float64 and len(m) == 2722 and np.isfinite(m).all()
    assert np.array_equal(m[0::2], -m[1::2]) and np.signbit(m[1]) and not np.signbit(m[0])   # every value in both signs, -0.0 included
    for x in (2.0 ** -1074, 2.0 ** -1022, 1.0, 60.0, 700.0, np.nextafter(700.0, np.inf), 750.0, np.nextafter(750.0, 0.0), 709.78, 745.13, mm.DBL_MAX, 53 * mm.LN2):
        assert x in m and -x in m
    assert np.array_equal(m, mm._grid())                       # the same grid every time it is built
    assert all(x not in m for x in mm.NONFINITE[:2])


def test_truths_agree_with_mpmath_at_60_digits():
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 60
    tiny = mpmath.mpf(2) ** -16000     # below it a longdouble truth may be subnormal or zero: held absolutely
    bar = mpmath.mpf(2) ** -60

    def hold(got, want, what):
        got = LD(got)
        man, ex = np.frexp(got)                                       # the longdouble, exactly: its 64 mantissa bits as two float64 halves
        hi = np.float64(man)
        got = (mpmath.mpf(float(hi)) + mpmath.mpf(float(np.float64(man - hi)))) * mpmath.mpf(2) ** int(ex)
        if abs(want) < tiny:
            assert abs(got) < tiny, what
        else:
            assert abs(got - want) <= bar * abs(want), (what, got, want)

    one = mpmath.mpf(1)
    for a in mm.MARGINS:
        x = mpmath.mpf(float(a))
        for y in (1.0, -1.0):
            hold(mm.mult_cls(a, y), -y / (one + mpmath.exp(y * x)), ("mult_cls", a, y))
        hold(mm.mult_bpr(a), -one / (one + mpmath.exp(x)), ("mult_bpr", a))
        hold(mm.logistic(a), one / (one + mpmath.exp(-x)), ("logistic", a))
        hold(mm.bpr_loss(a), max(-x, 0) + mpmath.log1p(mpmath.exp(-abs(x))), ("bpr_loss", a))


def test_truths_at_the_non_finite_margins():
    inf = float("inf")
    for y in (1.0, -1.0):
        m = mm.mult_cls([inf * y, -inf * y, float("nan")], y)
        assert m[0] == 0 and np.signbit(m[0]) == (y > 0) and m[1] == -y and np.isnan(m[2])
    assert mm.logistic(inf) == 1 and mm.logistic(-inf) == 0 and np.isnan(mm.logistic(float("nan")))
    assert mm.bpr_loss(inf) == 0 and mm.bpr_loss(-inf) == inf


# ------------------------------------------------------------------------------------------------------------------------------ the probe
@pytest.mark.parametrize("labels", ["plus", "minus", "alternating"])
@pytest.mark.parametrize("k", [0, 8])
def test_the_oracle_on_the_probe_meets_the_bar_and_moves_nothing_else(k, labels):
    a = probe_margins()
    y = label_sets(len(a))[labels]
    mult, ref, pr = oracle_probe(k, y)
    truth = mm.mult_cls(a, y)
    err = np.abs(mult[1:].astype(LD) - truth[1:]).astype(np.float64)
    i = int(np.argmax(err))
    print(f"oracle on the probe, k={k} {labels}: largest |mult - truth| = {err[i] / mm.BAR:.3f} of 2^-51 at a = {a[1 + i]!r}")
    assert err[i] <= mm.BAR
    assert mult[0] == 0.0 and ref["w"][0] == a[0]                                    # the spare row was not visited
    assert np.array_equal(ref["w"][0::3][1:], plain_update(a[1:], mult[1:]))           # w[3 j]: the plain formula on the same multiplier
    assert np.all(ref["w"][2::3] == 0.0) and np.all(ref["v"] == 0.0)                  # columns in no row; factor rows: 0 - mult * (0 * 1 - 0 * 1 * 1)
    exact = [oracle.grad_mult(oracle.params(), float(ai), float(yi))[0] for ai, yi in zip(a[1:], y[1:])]
    assert np.array_equal(mult[1:], np.array(exact))                                  # and w[3 j + 1] IS the multiplier, every bit


def test_the_oracle_on_the_non_finite_rows():
    pr0 = mm.probe_rows([mm.point_row(0.25)] + mm.NONFINITE_ROWS + [mm.point_row(3.0)])
    for y in (np.ones(pr0["n"]), -np.ones(pr0["n"])):
        mult, ref, pr = oracle_probe(8, y, probe=pr0)
        s = y[0]
        assert mult[1 if s > 0 else 2] == 0.0 and mult[2 if s > 0 else 1] == -s and np.isnan(mult[3])
        v = ref["v"].reshape(8, pr["p"])
        assert np.isnan(v[:, 9:12]).all()                                             # NaN in the NaN row's own three features ...
        assert np.all(v[:, :9] == 0.0) and np.all(v[:, 12:] == 0.0)                   # ... and nowhere else
        assert abs(mult[4] - float(mm.mult_cls(3.0, s))) <= mm.BAR


# ------------------------------------------------------------------------------------------- the model of the reassociated multiplier
def test_the_reassociated_multipliers_model_meets_its_bars():
    a, y, m = mm.re_model_table()
    truth = mm.mult_cls(a, y)
    err = np.abs(m.astype(LD) - truth).astype(np.float64)
    i = int(np.argmax(err))
    print(f"model of seq_grad_mult_re: largest |model - truth| = {err[i] / mm.BAR:.3f} of 2^-51 at a = {a[i]!r}, y = {y[i]:+.0f}")
    assert err[i] <= mm.BAR
    P = oracle.params()
    ref = np.array([oracle.grad_mult(P, float(ai), float(yi))[0] for ai, yi in zip(a, y)])
    d = np.abs(m - ref)
    j = int(np.argmax(d))
    print(f"                           largest |model - oracle| = {d[j]:.3e} (bar 2.3e-16) at a = {a[j]!r}, y = {y[j]:+.0f}")
    assert d[j] <= mm.RE_ABS_TO_ORACLE
    ulp, at, lab = mm.re_model_max_ulp()
    print(f"                           RE_MODEL_MAX_ULP = {ulp:.3f} at a = {at!r}, y = {lab:+.0f}")
    assert 0.5 <= ulp < 8.0     # a sanity window, not a bar: the kernel's comment says `2 ulp'; the GPU test holds the device to this figure + 1
    for x in mm.NONFINITE:
        for s in (1.0, -1.0):
            got, want = mm.mult_re_model(x, s), float(mm.mult_cls(x, s))
            # the clamp at 700 leaves 1 / (1 + e^700) = 9.9e-305 where the limit is 0: inside the absolute bar, not the limit's bits
            assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-304, (x, s, got, want)


def test_fma_is_rounded_once():
    e = 2.0 ** -30
    assert mm.fma(1.0 + e, 1.0 - e, -1.0) == -e * e and (1.0 + e) * (1.0 - e) - 1.0 == 0.0
    assert mm.fma(3.0, 1.0 / 3.0, -1.0) == -2.0 ** -54
    assert mm.fma(2.0, 3.0, -6.0) == 0.0 and not np.signbit(mm.fma(2.0, 3.0, -6.0))
    assert np.isnan(mm.fma(float("inf"), 0.0, 1.0)) and mm.fma(float("inf"), 1.0, 1.0) == float("inf")


# ------------------------------------------------------------------------------------------------------------------------------ regression
def test_the_regression_multiplier_of_the_oracle_is_mult_reg_bit_for_bit():
    P = oracle.params(task=oracle.REGRESSION, min_target=LO, max_target=HI)
    for p in reg_predictions():
        for y in REG_LABELS:
            got, clamped = oracle.grad_mult(P, p, y)
            want = mm.mult_reg(p, y, LO, HI)
            assert np.array([got]).tobytes() == np.array([want]).tobytes(), (p, y, got, want)
            assert LO <= clamped <= HI                                                 # the prediction is clamped in place, NaN included
    assert oracle.grad_mult(P, float("nan"), 0.0)[0] == HI                             # NaN -> max_target - y


def test_the_regression_clamp_through_the_oracles_learner():
    for fp32 in (False, True):
        pr, p, y = reg_probe(fp32)
        mult, ref, _ = oracle_probe(8, y, probe=pr, task=oracle.REGRESSION, min_target=LO, max_target=HI)
        want = np.array([mm.mult_reg(pi, yi, LO, HI) for pi, yi in zip(p[1:], y[1:])])
        assert np.array_equal(mult[1:], want)          # the clamp absorbs the NaN prediction: no NaN multiplier


# What the C++ library's std::min and std::max return when the second argument is NaN, asked of the library itself: for every (p as a bit pattern,
# y as text) on the command line the program prints the bits of -(y - std::max(lo, std::min(hi, p))).  The reference clamps with the bound as the
# FIRST argument of both calls (tests/margin_model.py's docstring has the order in prose).
_CXX = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv) {
  const double lo = -1.5, hi = 2.0;
  for (int i = 1; i + 1 < argc; i += 2) {
    const std::uint64_t in = std::strtoull(argv[i], nullptr, 16);
    double p;
    std::memcpy(&p, &in, sizeof p);
    const float y = std::strtof(argv[i + 1], nullptr);
    double t = std::min(hi, p);
    t = std::max(lo, t);
    const double m = -(y - t);
    std::uint64_t out;
    std::memcpy(&out, &m, sizeof out);
    std::printf("%016llx\n", (unsigned long long)out);
  }
  return 0;
}
"""


def _cxx_compiler():
    """a host C++ compiler: the oracle itself needs the C compiler of the same toolchain to build, so a machine that runs these tests has one"""
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    pytest.fail("no host C++ compiler found (tried g++, c++, clang++): the check of std::min / std::max on NaN cannot run")


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_mult_reg_is_what_std_min_and_std_max_compute(tmp_path, opt):
    """margin_model.mult_reg against the C++ standard library's own min and max, bound first, on every regression case: a NaN comes out of
    std::min(hi, NaN) as hi (NaN < hi is false, so the first argument is returned), hence the multiplier hi - y."""
    src, exe = tmp_path / "clamp.cpp", tmp_path / "clamp"
    src.write_text(_CXX)
    subprocess.run([_cxx_compiler(), "-std=c++11", opt, "-o", str(exe), str(src)], check=True, capture_output=True)
    cases = [(p, y) for p in reg_predictions() for y in REG_LABELS]
    args = []
    for p, y in cases:
        args += ["%016x" % int(np.array([p]).view(np.uint64)[0]), repr(y)]
    out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.split()
    want = ["%016x" % int(np.array([mm.mult_reg(p, y, LO, HI)]).view(np.uint64)[0]) for p, y in cases]
    assert out == want
    nan_rows = [o for (p, y), o in zip(cases, out) if p != p]
    assert nan_rows == ["%016x" % int(np.array([-(y - HI)]).view(np.uint64)[0]) for y in REG_LABELS]


# ------------------------------------------------------------------------------------------------------------------------------ evaluate
def test_log_likelihood_is_nan_exactly_when_a_probability_is_one_whatever_the_label():
    """core/Evaluation.h:80-89: (1 + y) log(p + 1e-20) + (1 - y) log(1 - p - 1e-20).  p = 1 makes the second logarithm log(-1e-20) = NaN whatever
    its factor (0 * NaN); p = 0 makes 1 - 0 - 1e-20 = 1 and log(0 + 1e-20) finite: only p == 1 (and a NaN p) makes the sum NaN."""
    ev = lambda p, y: oracle.evaluate(oracle.CLASSIFICATION, oracle.LL, np.array(p, np.float64), np.array(y, np.float32))
    base_p, base_y = [0.25, 0.5, 0.75], [1.0, -1.0, 1.0]
    assert np.isfinite(ev(base_p, base_y))
    for y in (1.0, -1.0):
        assert np.isnan(ev(base_p + [1.0], base_y + [y]))               # 1 - 1 - 1e-20 < 0
        assert np.isfinite(ev(base_p + [0.0], base_y + [y]))            # log(1e-20) and log(1 - 1e-20) = log(1)
        assert np.isfinite(ev(base_p + [float(np.nextafter(1.0, 0.0))], base_y + [y]))
    assert np.isnan(ev(base_p + [float("nan")], base_y + [1.0]))


def test_accuracy_counts_a_probability_of_one_half_for_positive_labels_only():
    ev = lambda p, y: oracle.evaluate(oracle.CLASSIFICATION, oracle.ACC, np.array(p, np.float64), np.array(y, np.float32))
    assert ev([0.5, 0.5], [1.0, -1.0]) == 0.5
    assert ev([0.5], [1.0]) == 1.0 and ev([0.5], [-1.0]) == 0.0
    assert ev([float(np.nextafter(0.5, 0.0))], [-1.0]) == 1.0
