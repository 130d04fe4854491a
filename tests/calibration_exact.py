"""The calibration figures of cdc_eval_calibration as exact rationals (helper of tests/test_calibration_cpu.py and
tests/test_gpu_calibration.py; not a test).  The contract, per segment (one domain's rows, or all rows) of m rows with predictions
p (float32 in [0, 1], -0.0 counts as 0) and labels y in {0, 1}, K = n_bins:

    q = rint(p * 2^32)  (to even), an integer in [0, 2^32]; every sum of predictions is a sum of q
    mean_pred = sum q / (m 2^32)    ctr = positives / m    pcoc = sum q / (positives 2^32)    brier = sum (q - y 2^32)^2 / (m 2^64)
    equal-width bin of a row: min(K - 1, floor(p K))
    equal-mass bin b: the positions [floor(b m / K), floor((b + 1) m / K)) of the rows sorted ascending by (p, y)
    per bin: count, positives, mean_pred = sum q / (count 2^32), pos_rate = positives / count, pred_min, pred_max
    ece = sum_b |sum q_b - positives_b 2^32| / (m 2^32)    mce = max_b |sum q_b - positives_b 2^32| / (count_b 2^32), b non-empty

Two forms: `calibration_rows` counts with numpy (sums as Python ints, no numpy integer can overflow) so that it reaches the GPU
tests' sizes; `calibration_rows_slow` walks the rows one by one with fractions.Fraction and Python's own sort — quantisation and
both bin rules included — and tests/test_calibration_cpu.py holds the first to it.  A value is a Fraction (an int for a count, a
numpy float32 for pred_min / pred_max), or None where the contract says NaN.
"""
from fractions import Fraction

import numpy as np

ONE = 1 << 32
CHUNK = 1 << 20
SEGMENT_FIELDS = ("mean_pred", "ctr", "pcoc", "brier", "ece", "mce", "ece_q", "mce_q")
TABLE_FIELDS = ("count", "positives", "mean_pred", "pos_rate", "pred_min", "pred_max")


def _f32(p):
    return np.asarray(p, dtype=np.float32) + np.float32(0.0)               # -0.0 -> +0.0


def quantise(p):
    """int64 [n]: rint(p * 2^32).  The product only moves the exponent of the float64, numpy's rint rounds half to even."""
    return np.rint(_f32(p).astype(np.float64) * float(ONE)).astype(np.int64)


def width_bins(p, K):
    """int64 [n]: min(K - 1, floor(p K)); float32 times K <= 1024 has at most 35 significant bits: exact in float64"""
    return np.minimum(np.floor(_f32(p).astype(np.float64) * float(K)).astype(np.int64), K - 1)


def _int_sum(x):
    """sum of a non-negative int64 array with entries <= 2^32 as a Python int"""
    return sum(int(x[i:i + CHUNK].sum()) for i in range(0, len(x), CHUNK))


def _int_sum_sq(x):
    """sum of squares of such an array: 16-bit halves, a chunk's partial sums stay below 2^53"""
    total = 0
    for i in range(0, len(x), CHUNK):
        hi, lo = x[i:i + CHUNK] >> 16, x[i:i + CHUNK] & 0xffff
        total += (int((hi * hi).sum()) << 32) + (int((hi * lo).sum()) << 17) + int((lo * lo).sum())
    return total


def _table(bounds, p, q, y):
    """rows sorted by (p, y); bin b = positions [bounds[b], bounds[b + 1]) -> (table, ece numerator, mce)"""
    cq = np.concatenate([[0], np.cumsum(q)])                              # < 2^31 * 2^32: no overflow
    cy = np.concatenate([[0], np.cumsum(y)])
    t = {k: [] for k in TABLE_FIELDS}
    gap_sum, mce = 0, None
    for b in range(len(bounds) - 1):
        lo, hi = int(bounds[b]), int(bounds[b + 1])
        cnt, sq, ps = hi - lo, int(cq[hi] - cq[lo]), int(cy[hi] - cy[lo])
        t["count"].append(cnt)
        t["positives"].append(ps)
        t["mean_pred"].append(Fraction(sq, cnt * ONE) if cnt else None)
        t["pos_rate"].append(Fraction(ps, cnt) if cnt else None)
        t["pred_min"].append(p[lo] if cnt else None)
        t["pred_max"].append(p[hi - 1] if cnt else None)
        if cnt:
            gap = abs(sq - ps * ONE)
            gap_sum += gap
            g = Fraction(gap, cnt * ONE)
            mce = g if mce is None or g > mce else mce
    return t, gap_sum, mce


def calibration_rows(y, p, n_bins):
    """One set of rows -> dict(rows, positives, sum_q, the SEGMENT_FIELDS, table, table_q)"""
    K = int(n_bins)
    y = (np.asarray(y) != 0).astype(np.int64)
    p = _f32(p)
    m = len(y)
    order = np.lexsort((y, p))                                             # ascending by p, then by y
    y, p = y[order], p[order]
    q = quantise(p)
    bw = width_bins(p, K)
    assert m == 0 or (p[0] >= 0 and p[-1] <= 1 and np.all(np.diff(bw) >= 0))
    P, sum_q = int(y.sum()), _int_sum(q)
    tw, gap_w, mce_w = _table(np.searchsorted(bw, np.arange(K + 1), side="left"), p, q, y)
    tq, gap_q, mce_q = _table([(b * m) // K for b in range(K + 1)], p, q, y)
    r = {"rows": m, "positives": P, "sum_q": sum_q, "table": tw, "table_q": tq}
    if m == 0:
        r.update({k: None for k in SEGMENT_FIELDS})
        return r
    r.update({"mean_pred": Fraction(sum_q, m * ONE), "ctr": Fraction(P, m), "pcoc": Fraction(sum_q, P * ONE) if P else None,
              "brier": Fraction(_int_sum_sq(np.abs(q - y * ONE)), m * ONE * ONE),
              "ece": Fraction(gap_w, m * ONE), "mce": mce_w, "ece_q": Fraction(gap_q, m * ONE), "mce_q": mce_q})
    return r


def calibration_rows_slow(y, p, n_bins):
    """The same, every row by itself in Fractions: the definitions as they are written"""
    K = int(n_bins)
    rows = []
    for yi, pi in zip(y, np.asarray(p, dtype=np.float32)):
        f = Fraction(float(pi))                                            # -0.0 -> 0
        q = round(f * ONE)                                                 # Python rounds a Fraction half to even
        assert 0 <= q <= ONE
        rows.append((f, int(yi != 0), q, np.float32(pi) + np.float32(0.0)))
    rows.sort(key=lambda r: (r[0], r[1]))
    m = len(rows)
    bins_w = [[] for _ in range(K)]
    bins_q = [[] for _ in range(K)]
    for r in rows:
        bins_w[min(K - 1, int(r[0] * K))].append(r)                        # int() of a non-negative Fraction is floor
    for b in range(K):
        bins_q[b] = rows[(b * m) // K:((b + 1) * m) // K]

    def table(bins):
        t = {k: [] for k in TABLE_FIELDS}
        gaps = []
        for rs in bins:
            cnt, sq, ps = len(rs), sum(r[2] for r in rs), sum(r[1] for r in rs)
            t["count"].append(cnt)
            t["positives"].append(ps)
            t["mean_pred"].append(Fraction(sq, cnt * ONE) if cnt else None)
            t["pos_rate"].append(Fraction(ps, cnt) if cnt else None)
            t["pred_min"].append(rs[0][3] if cnt else None)
            t["pred_max"].append(rs[-1][3] if cnt else None)
            if cnt:
                gaps.append((abs(sq - ps * ONE), cnt))
        return t, sum(g for g, _ in gaps), max((Fraction(g, c * ONE) for g, c in gaps), default=None)

    tw, gap_w, mce_w = table(bins_w)
    tq, gap_q, mce_q = table(bins_q)
    P, sum_q = sum(r[1] for r in rows), sum(r[2] for r in rows)
    r = {"rows": m, "positives": P, "sum_q": sum_q, "table": tw, "table_q": tq}
    if m == 0:
        r.update({k: None for k in SEGMENT_FIELDS})
        return r
    r.update({"mean_pred": Fraction(sum_q, m * ONE), "ctr": Fraction(P, m), "pcoc": Fraction(sum_q, P * ONE) if P else None,
              "brier": Fraction(sum((r[2] - r[1] * ONE) ** 2 for r in rows), m * ONE * ONE),
              "ece": Fraction(gap_w, m * ONE), "mce": mce_w, "ece_q": Fraction(gap_q, m * ONE), "mce_q": mce_q})
    return r


def calibration_exact(y, p, n_bins, domain=None, n_domain=1, rows_fn=calibration_rows):
    """Every figure of cdc_eval_calibration: a list with n_domain + 1 entries (domains 0..n_domain-1, then ALL rows) of
    calibration_rows' dictionaries."""
    y, p = np.asarray(y), np.asarray(p, dtype=np.float32)
    everything = rows_fn(y, p, n_bins)
    if domain is None:                                                     # n_domain == 1: the one domain is every row
        return [everything] * (n_domain + 1)
    return [rows_fn(y[np.asarray(domain) == d], p[np.asarray(domain) == d], n_bins) for d in range(n_domain)] + [everything]


def as_float(v):
    return float("nan") if v is None else float(v)
