"""The numpy model of fmx_neighbors (include/fmx.h), the yardstick of tests/test_gpu_neighbors.py: steps 2 to 6 of the
contract run literally.  The projections come in as float64 arrays (exact widenings of the state type) and the fma chain as a function, as in
tests/diversify_model.py, whose chain and norms it takes: `chain_exact` for the Fraction emulation of the kernel's chain, `chain_dot` where
every chain is exact anyway.  tests/test_neighbors_cpu.py checks it against a brute-force double loop."""
import numpy as np

from tests.diversify_model import QNAN, chain_dot, chain_exact, norms_inv  # noqa: F401  (re-exported for the tests)

SIM_COSINE, SIM_DOT = 0, 1


def scores(sq, si, metric, chain, inv_q=None, inv_i=None):
    """steps 2-4: float64[n_q, n_i], the score of every (query, item) pair.  sq float64[n_q, k], si float64[n_i, k]"""
    nq, ni = len(sq), len(si)
    out = np.zeros((nq, ni))
    if metric == SIM_COSINE:
        inv_q = norms_inv(sq, chain) if inv_q is None else inv_q                # 3
        inv_i = norms_inv(si, chain) if inv_i is None else inv_i
    for q in range(nq):
        if not ni:
            break
        d = np.asarray(chain(si, sq[q]), np.float64).reshape(ni)                 # 2 (a product commutes, so the chain is d(q, i))
        if metric == SIM_DOT:
            out[q] = d
        elif inv_q[q] != 0.0:
            with np.errstate(all="ignore"):
                out[q] = np.where(inv_i != 0.0, (d * inv_q[q]) * inv_i, 0.0)     # 4: the query's inverse norm first
    return out


def order(score, eligible):
    """step 5 for one query: the eligible item indices in the order -- a higher score first (-0 = +0), equal scores by the lower index, NaN last"""
    idx = np.asarray(eligible, np.int64)
    s = score[idx]
    nan = np.isnan(s)
    return idx[np.lexsort((idx, np.where(nan, 0.0, -s), nan))]                   # keys last to first


def select(score, top_k, skip_self=False, row0=0):
    """steps 5-6 on a score matrix [n_q, n_i] whose row q is query row row0 + q: (index int64[n_q, top_k], score float64[n_q, top_k])"""
    nq, ni = score.shape
    oi, os_ = np.full((nq, top_k), -1, np.int64), np.full((nq, top_k), QNAN)
    for q in range(nq):
        elig = np.arange(ni)
        if skip_self:
            elig = elig[elig != row0 + q]                                        # 6
        o = order(score[q], elig)[:top_k]
        oi[q, :len(o)], os_[q, :len(o)] = o, score[q, o]
    return oi, os_


def neighbors(sq, si, top_k, metric, chain, skip_self=False, row0=0, inv_q=None, inv_i=None):
    """the whole call: queries sq (row q is query row row0 + q of its matrix) against items si"""
    return select(scores(sq, si, metric, chain, inv_q, inv_i), top_k, skip_self, row0)
