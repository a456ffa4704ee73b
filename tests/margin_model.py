"""The margins at which the transfer functions between a raw score and a gradient, a probability or a loss term saturate, their truths in
extended precision, a step-by-step restatement of the reassociated learner's hand-written multiplier, and the probe matrices that let a test read
one row's multiplier back out of a parameter table.  No GPU and nothing of the engine: numpy, the standard library.

MARGINS is a fixed, ordered float64 grid, every value in both signs: zeros and the smallest magnitudes, the integers to 60, 1 024 log-uniform draws
in [2^-10, 2^5], the ties of rint(x log2 e) (n ln2 / 2 and its neighbours), the margins around which 1 + exp(a) stops seeing its smaller term
(52..54 ln 2: 36.04, 36.74, 37.43), the clamps of the reassociated multiplier (-750 and 700) with their neighbours, the margins at which exp
overflows (709.78) or enters and leaves the subnormals (708.39, 744.44, 745.13), and magnitudes up to DBL_MAX.  NONFINITE is kept apart so that
a failure on it is a test of its own.

The truths are np.longdouble (64 mantissa bits on x86) and written without cancellation:
    mult_cls(a, y) = -y / (1 + exp(y a))         the reference's -y (1 - 1 / (1 + exp(-y a))), solver/SGD_Learner.h:188
    mult_bpr(d)    = -1 / (1 + exp(d))
    logistic(z)    = 1 / (1 + exp(-z))
    bpr_loss(d)    = max(-d, 0) + log1p(exp(-|d|))
mult_reg is no approximation at all.  The reference's regression branch (solver/SGD_Learner.h:184-186) clamps the prediction with the C++ library's min
and max, the bound given FIRST both times -- the upper bound, then the lower -- and takes minus (label - clamped prediction).  The standard
defines
    std::min(a, b) = (b < a) ? b : a,      std::max(a, b) = (a < b) ? b : a,
both returning their FIRST argument where the comparison is false.  A NaN prediction therefore leaves std::min(upper bound, NaN) = the upper bound
and the multiplier max_target - y -- what fmin / fmax give on the device.  (tests/test_margin_cpu.py asks the host's C++ library the same question
and holds mult_reg to the answer.)"""
import functools
import math
import struct
from fractions import Fraction

import numpy as np

LD = np.longdouble
LN2 = math.log(2.0)
DBL_MAX = float(np.finfo(np.float64).max)
BAR = 2.0 ** -51            # the absolute bar of an fp64 multiplier (tests/test_margin_cpu.py derives it)
RE_ABS_TO_ORACLE = 2.3e-16  # the reassociated multiplier against the reference's expression (the kernel comment's figure)


def _neighbours(x):
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


def _grid():
    pos = [0.0, 2.0 ** -1074, 2.0 ** -1022, 2.0 ** -60, 2.0 ** -53, 2.0 ** -30]
    pos += [float(i) for i in range(1, 61)]
    rng = np.random.default_rng(20240519)
    pos += [float(x) for x in 2.0 ** rng.uniform(-10.0, 5.0, 1024)]
    for n in range(1, 81):                       # the ties of rint(x log2 e)
        pos += _neighbours(n * LN2 / 2.0)
    for n in (52, 53, 54):                       # 1 + exp(a) loses exp(-a): 36.04, 36.74, 37.43
        pos += _neighbours(n * LN2)
    pos += [100.0, 212.834, 500.0, 699.9]
    pos += _neighbours(700.0)
    pos += [708.39, 709.78, 709.79, 710.0, 744.44, 745.13, 745.14]
    pos += _neighbours(750.0)
    pos += [751.0, 1e3, 1e10, 1e300, DBL_MAX]
    out = np.empty(2 * len(pos), np.float64)
    out[0::2] = pos
    out[1::2] = [-x for x in pos]
    return out


MARGINS = _grid()
MARGINS.setflags(write=False)
NONFINITE = [float("inf"), float("-inf"), float("nan")]


# ------------------------------------------------------------------------------------------------------------------------------- truths
def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


def mult_cls(a, y):
    """-y / (1 + exp(y a)), longdouble; exp's overflow gives the signed zero the limit has, NaN stays NaN."""
    a, y = _ld(a), _ld(y)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return -y / (LD(1) + np.exp(y * a))


def mult_bpr(d):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return LD(-1) / (LD(1) + np.exp(_ld(d)))


def logistic(z):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return LD(1) / (LD(1) + np.exp(-_ld(z)))


def bpr_loss(d):
    d = _ld(d)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.maximum(-d, LD(0)) + np.log1p(np.exp(-np.abs(d)))


def mult_reg(yhat, y, lo, hi):
    """The reference's regression multiplier for ONE prediction, float64 and exact: std::min(hi, yhat) then std::max(lo, .) as comparisons
    (see the module's docstring), then -(y - yhat) with y a float widened to double.  NaN -> hi - y."""
    yhat, lo, hi = float(yhat), float(lo), float(hi)
    t = yhat if yhat < hi else hi       # std::min(hi, yhat) = (yhat < hi) ? yhat : hi
    t = t if lo < t else lo             # std::max(lo, t)    = (lo < t) ? t : lo
    return -(float(np.float32(y)) - t)


# ------------------------------------------------------------------------------------------------------ seq_grad_mult_re, step by step
def _bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def fma(a, b, c):
    """a b + c rounded once: exact rational arithmetic, and float(Fraction) is correctly rounded (to nearest, ties to even)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c if (a == 0 or b == 0) and c == 0 else 0.0   # an exact cancellation is +0 to nearest; zeros keep the sign IEEE gives them
    return float(r)


# fm_seq_kernels.hip: seq_grad_mult_re's constants by their bit patterns
_LOG2E, _LN2_HI, _LN2_LO = _bits(0x3ff71547652b82fe), _bits(0xbfe62e42fefa39ef), _bits(0xbc7abc9e3b39803f)
_C2, _C3 = _bits(0x3fe000000000000b), _bits(0x3fc5555555555511)
_C4, _C5 = _bits(0x3fa55555555502a1), _bits(0x3f81111111122322)
_C6, _C7 = _bits(0x3f56c16c1852b7b0), _bits(0x3f2a01a014761f6e)
_C8, _C9 = _bits(0x3efa01997c89e6b0), _bits(0x3ec71dee623fde64)
_CA, _CB = _bits(0x3e928af3fca7ab0c), _bits(0x3e5ade156a5dcb37)


def mult_re_model(a_in, y):
    """seq_grad_mult_re(y_hat = a_in, y) for one finite or non-finite prediction: the kernel's operations in its order, every fma rounded once,
    everything else float64.  The reciprocal seed is the correctly rounded 1 / d (the device's v_rcp_f64 seed is another value of about 2^-22
    relative error; the two Newton steps are applied to either)."""
    yd = float(np.float32(y))
    a = yd * float(a_in)
    if a != a:
        return -yd * a
    x = min(max(a, -750.0), 700.0)
    n = float(np.rint(x * _LOG2E))
    r = fma(n, _LN2_HI, x)
    r = fma(n, _LN2_LO, r)
    r2 = r * r
    r4 = r2 * r2
    r8 = r4 * r4
    p01 = 1.0 + r
    p23 = fma(_C3, r, _C2)
    p45 = fma(_C5, r, _C4)
    p67 = fma(_C7, r, _C6)
    p89 = fma(_C9, r, _C8)
    pab = fma(_CB, r, _CA)
    q0, q1, q2 = fma(p23, r2, p01), fma(p67, r2, p45), fma(pab, r2, p89)
    t = math.ldexp(fma(q2, r8, fma(q1, r4, q0)), int(n))
    d = 1.0 + t
    xr = 1.0 / d
    xr = fma(xr, fma(-d, xr, 1.0), xr)
    xr = fma(xr, fma(-d, xr, 1.0), xr)
    return -yd * xr


def ulp_error(got, truth):
    """|got - truth| in units of the float64 spacing at |truth| (truth longdouble)."""
    t64 = np.abs(np.asarray(truth, LD)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(got, np.float64).astype(LD) - np.asarray(truth, LD)) / np.spacing(t64).astype(LD)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def re_model_table():
    """(margins, labels, model values) of mult_re_model over MARGINS x {+1, -1}: computed once per process."""
    a = np.concatenate([MARGINS, MARGINS])
    y = np.concatenate([np.ones(len(MARGINS)), -np.ones(len(MARGINS))])
    m = np.array([mult_re_model(ai, yi) for ai, yi in zip(a, y)], np.float64)
    return a, y, m


@functools.lru_cache(maxsize=None)
def re_model_max_ulp():
    """(RE_MODEL_MAX_ULP, margin, label): the model's largest relative error in ulp over the margins with |a| <= 700 (inside the clamps) and a
    truth of at least 2^-1000."""
    a, y, m = re_model_table()
    truth = mult_cls(a, y)
    keep = (np.abs(a) <= 700.0) & (np.abs(truth) >= LD(2.0) ** -1000)
    u = np.where(keep, ulp_error(m, truth), 0.0)
    i = int(np.argmax(u))
    return float(u[i]), float(a[i]), float(y[i])


# ---------------------------------------------------------------------------------------------------------------------- probe matrices
def probe_matrix(margins, layout="point"):
    """A CSR (dict rp, col, val, p, w, n) in which the multiplier of every row can be read back exactly.

    layout "point": row j holds column 3 j with x = 1 and weight margins[j], and column 3 j + 1 with x = 1 and weight 0 (column 3 j + 2 is in no
    row).  With all factor rows zero y_hat = margins[j] + 0 in any association, every row owns its columns, and one step of rate 1 without decay
    leaves w[3 j + 1] = 0 - mult_j.

    layout "pair" (ranking): row 2 t holds (3 t: weight margins[t]) and (3 t + 1: weight 0), row 2 t + 1 holds (3 t + 2: weight 0): the pair's
    difference is margins[t] - 0, and the two zero-weight features receive m0 and -m0 as their gradients."""
    a = np.asarray(margins, np.float64)
    T = len(a)
    w = np.zeros(3 * T)
    w[0::3] = a
    if layout == "point":
        rp = 2 * np.arange(T + 1, dtype=np.int64)
        col = np.stack([3 * np.arange(T), 3 * np.arange(T) + 1], axis=1).ravel().astype(np.uint32)
        n = T
    elif layout == "pair":
        rp = np.zeros(2 * T + 1, np.int64)
        rp[1::2] = 3 * np.arange(T) + 2
        rp[2::2] = 3 * np.arange(T) + 3
        col = np.arange(3 * T, dtype=np.uint32)
        n = 2 * T
    else:
        raise ValueError(layout)
    return dict(rp=rp, col=col, val=np.ones(len(col), np.float32), p=3 * T, w=w, n=n)


def probe_rows(rows):
    """A small probe from explicit rows: rows[j] is a list of one to three (weight, x) entries, entry i at column 3 j + i.  Same dict as probe_matrix."""
    rp, col, val = [0], [], []
    w = np.zeros(3 * len(rows))
    for j, r in enumerate(rows):
        assert 1 <= len(r) <= 3
        for i, (wt, x) in enumerate(r):
            w[3 * j + i] = wt
            col.append(3 * j + i)
            val.append(x)
        rp.append(len(col))
    return dict(rp=np.array(rp, np.int64), col=np.array(col, np.uint32), val=np.array(val, np.float32), p=3 * len(rows), w=w, n=len(rows))


def point_row(a):
    return [(float(a), 1.0), (0.0, 1.0)]


# Non-finite MARGINS from FINITE parameters (fp64 tables): 1e300 x 1e10 overflows in the forward's own sum.  The read-back feature (column 3 j + 1,
# x = 1, weight 0) is the second entry as in every other row.  An infinite PARAMETER is another matter and not a case here: the mini-batch forward
# pads its gather rounds with (the row's first column, x = +0), so an infinite weight meets 0 x inf there.
BIG_W, BIG_X = 1e300, 1e10
POS_INF_ROW = [(BIG_W, BIG_X), (0.0, 1.0)]
NEG_INF_ROW = [(-BIG_W, BIG_X), (0.0, 1.0)]
NAN_ROW = [(BIG_W, BIG_X), (0.0, 1.0), (-BIG_W, BIG_X)]
NONFINITE_ROWS = [POS_INF_ROW, NEG_INF_ROW, NAN_ROW]          # the margins of NONFINITE, in its order
# fp32 tables cannot overflow the forward's fp64 sums from finite parameters: there NaN is a stored weight (three entries, like NAN_ROW)
NAN_WEIGHT_ROW = [(float("nan"), 1.0), (0.0, 1.0), (0.0, 1.0)]
