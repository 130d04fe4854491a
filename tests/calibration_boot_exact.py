"""The contract of cdc_eval_calibration_bootstrap without a device (helper of tests/test_calibration_boot_cpu.py and
tests/test_gpu_calibration_boot.py; not a test).

Replicate r gives row i the weight w_i = bootstrap_exact.weights(seed, r, cluster_i) (cluster = the row index without a cluster
column), and its figures are cdc_eval_calibration's on the multiset in which row i appears w_i times.  Per segment (domain
0..n_domain-1, then ALL rows), with q = rint(p * 2^32) and K = n_bins:

    W = sum w   Wp = sum w y   SQ = sum w q   SE2 = sum w (q - y 2^32)^2
    pcoc = SQ / (Wp 2^32)    brier = SE2 / (W 2^64)    ece = sum_b |SQ_b - Wp_b 2^32| / (W 2^32)
    equal-width bin of a row: min(K - 1, floor(p K))
    equal-mass bins: rows ordered by (p, y); row i holds the expanded positions [R_i, R_i + w_i), R_i the weight in front of it;
        bin b is the expanded positions [floor(b W / K), floor((b + 1) W / K)); a row gives a bin as many copies as lie in it

Two independent forms: `by_expansion` repeats the rows (np.repeat) and hands them to calibration_exact.calibration_rows;
`direct` writes the weighted formulas out with Python integers and Fractions, the split of a row's copies over the mass bins
included.  Both return [replicate][segment] dictionaries (W, Wp: ints; pcoc, brier, ece, ece_q: a Fraction, or None where the
contract says NaN).
"""
from fractions import Fraction

import numpy as np

import bootstrap_exact as B
from calibration_exact import ONE, calibration_rows, quantise, width_bins

FIGURES = ("pcoc", "brier", "ece", "ece_q")


def clip01(p):
    """the prediction as cdc_eval_calibration counts it: NaN and values below 0 as 0, values above 1 as 1"""
    p = np.asarray(p, dtype=np.float32)
    return np.where(p > 1, np.float32(1), np.where(p >= 0, p, np.float32(0))).astype(np.float32)


def _inputs(y, p, cluster, domain, n_domain):
    y = (np.asarray(y) != 0).astype(np.int64)
    p = np.asarray(p, dtype=np.float32) + np.float32(0.0)
    n = len(y)
    c = np.arange(n, dtype=np.int64) if cluster is None else np.asarray(cluster).astype(np.int64)
    masks = [np.ones(n, dtype=bool) if d == n_domain or domain is None else np.asarray(domain) == d for d in range(n_domain + 1)]
    return y, p, c, masks


def rep_weights(seed, r, n, cluster=None):
    c = np.arange(n, dtype=np.int64) if cluster is None else np.asarray(cluster).astype(np.int64)
    return B.weights(seed, r, c)


def _expanded_segment(y, p, w, K):
    e = calibration_rows(np.repeat(y, w), np.repeat(p, w), K)
    return {"W": e["rows"], "Wp": e["positives"], **{k: e[k] for k in FIGURES}}


def _direct_segment(y, p, w, K):
    rows = sorted((Fraction(float(pi)), int(yi), int(qi), int(bi), int(wi))
                  for pi, yi, qi, bi, wi in zip(p, y, quantise(p), width_bins(p, K), w))       # by (p, y): ties are identical rows
    W = sum(r[4] for r in rows)
    Wp = sum(r[4] * r[1] for r in rows)
    out = {"W": W, "Wp": Wp, "pcoc": None, "brier": None, "ece": None, "ece_q": None}
    if W == 0:
        return out
    SQ = sum(r[4] * r[2] for r in rows)
    SE2 = sum(r[4] * (r[2] - r[1] * ONE) ** 2 for r in rows)
    sq_w, wp_w = [0] * K, [0] * K
    sq_q, wp_q = [0] * K, [0] * K
    bounds = [(b * W) // K for b in range(K + 1)]
    R, b = 0, 0
    for _, yi, qi, bi, wi in rows:
        sq_w[bi] += wi * qi
        wp_w[bi] += wi * yi
        lo, hi = R, R + wi                                                 # the row's expanded positions
        while lo < hi:
            while bounds[b + 1] <= lo:                                     # the bin that holds position lo (empty bins are passed)
                b += 1
            copies = min(hi, bounds[b + 1]) - lo
            sq_q[b] += copies * qi
            wp_q[b] += copies * yi
            lo += copies
        R = hi
    out["pcoc"] = Fraction(SQ, Wp * ONE) if Wp else None
    out["brier"] = Fraction(SE2, W * ONE * ONE)
    out["ece"] = Fraction(sum(abs(a - c * ONE) for a, c in zip(sq_w, wp_w)), W * ONE)
    out["ece_q"] = Fraction(sum(abs(a - c * ONE) for a, c in zip(sq_q, wp_q)), W * ONE)
    return out


def _run(segment_fn, y, p, n_bins, cluster, seed, n_rep, domain, n_domain, weight_fn):
    y, p, c, masks = _inputs(y, p, cluster, domain, n_domain)
    out = []
    for r in range(n_rep):
        w = np.asarray(weight_fn(seed, r, c), dtype=np.int64)
        out.append([segment_fn(y[mk], p[mk], w[mk], int(n_bins)) for mk in masks])
    return out


def by_expansion(y, p, n_bins=10, cluster=None, seed=0, n_rep=1, domain=None, n_domain=1, weight_fn=B.weights):
    """-> [replicate][segment] dict(W, Wp, pcoc, brier, ece, ece_q): the rows repeated by their weights, then calibration_rows"""
    return _run(_expanded_segment, y, p, n_bins, cluster, seed, n_rep, domain, n_domain, weight_fn)


def direct(y, p, n_bins=10, cluster=None, seed=0, n_rep=1, domain=None, n_domain=1, weight_fn=B.weights):
    """the same from the weighted formulas in Python integers, a row's copies split over the mass bins one bin at a time"""
    return _run(_direct_segment, y, p, n_bins, cluster, seed, n_rep, domain, n_domain, weight_fn)


def as_array(res, field):
    """[n_rep, n_seg] float64 of one field, NaN for None"""
    return np.array([[float("nan") if s[field] is None else float(s[field]) for s in rep] for rep in res], dtype=np.float64)
