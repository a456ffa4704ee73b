"""Builders shared by tests/test_margin_cpu.py and tests/test_gpu_margins.py: the regression cases, the label sets, the probes over the grid of
tests/margin_model.py and the oracle's one pass over a probe.  No GPU."""
import numpy as np

import oracle
from tests import margin_model as mm

LO, HI = -1.5, 2.0
REG_LABELS = [-1.5, 0.0, 2.0, 7.25]


def reg_predictions():
    nb = lambda x: [float(np.nextafter(x, -np.inf)), x, float(np.nextafter(x, np.inf))]
    return nb(LO) + nb(HI) + [0.0, -0.0, 1e300, -1e300, float("inf"), float("-inf"), float("nan")]


def label_sets(n):
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return {"plus": np.ones(n), "minus": -np.ones(n), "alternating": alt}


def probe_margins():
    """The reference never visits row 0 at random_step = 1 (SURVEY A-2): row 0 is a spare row, rows 1 .. N hold MARGINS."""
    return np.concatenate([[0.25], mm.MARGINS])


def oracle_probe(k, y, margins=None, task=oracle.CLASSIFICATION, probe=None, **kw):
    """One pass of the reference-order SGD learner over the probe (rows 1 .. N once each): (mult read back from w[3 j + 1], result dict, probe)."""
    pr = probe if probe is not None else mm.probe_matrix(probe_margins() if margins is None else np.asarray(margins, np.float64))
    P = oracle.params(task=task, k=k, k0=False, learn_rate=1.0, random_step=1, **kw)
    X = oracle.Matrix(pr["rp"], pr["col"], pr["val"], pr["p"])
    with np.errstate(all="ignore"):
        ref = oracle.sgd_learn(P, X, np.asarray(y, np.float32), 0.0, pr["w"], np.zeros(k * pr["p"]), pr["n"] - 1)
    assert ref["iters"] == pr["n"] - 1
    return -ref["w"][1::3], ref, pr


def plain_update(a, mult):
    """w[3 j] after the row's one step at rate 1 and decay 0, by the reference's two statements: w -= 1 * mult * 1; w -= 1 * 0 * w."""
    with np.errstate(all="ignore"):
        t = a - mult
        return t - 0.0 * t


def nonfinite_probe(special=True):
    """(probe, rows of the +inf, -inf and NaN margins): a spare row 0, forty ordinary rows, the three non-finite margins made from finite
    parameters (margin_model.NONFINITE_ROWS), twenty-seven ordinary rows; special=False puts ordinary rows in their place."""
    before, after = mm.MARGINS[:80:2], mm.MARGINS[1200:1280:3]
    mid = mm.NONFINITE_ROWS if special else [mm.point_row(0.5)] * 3
    rows = [mm.point_row(0.25)] + [mm.point_row(a) for a in before] + mid + [mm.point_row(a) for a in after]
    return mm.probe_rows(rows), np.arange(41, 44)


def reg_probe(fp32=False):
    """(probe, predictions, labels): a spare row 0, then every prediction of reg_predictions() under every label.  The non-finite predictions
    come from finite parameters (margin_model.NONFINITE_ROWS); fp32 tables cannot reach +-inf that way and +-1e300 is no float: they keep the
    finite predictions that are floats' values, and NaN as a stored weight."""
    rows, preds, labels = [mm.point_row(0.25)], [0.25], [0.0]
    special = dict(zip(["inf", "-inf", "nan"], mm.NONFINITE_ROWS))
    for y in REG_LABELS:
        for p in reg_predictions():
            if fp32 and (np.isinf(p) or abs(p) > 3e38):
                continue
            key = repr(float(p))
            rows.append(mm.NAN_WEIGHT_ROW if fp32 and key == "nan" else special.get(key, mm.point_row(p)))
            preds.append(float(p)); labels.append(y)
    return mm.probe_rows(rows), np.array(preds), np.array(labels)
