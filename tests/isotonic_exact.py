"""Exact host restatements of per-segment isotonic regression of 0/1 labels on float32 scores (helper, not a test).

A fit is a list of blocks (x_lo, x_hi, count, positives) in ascending score order: x_lo / x_hi numpy float32, count / positives
Python ints, the block's value positives / count, strictly increasing along the list.  Every comparison of two means is a
comparison of integer products; nothing is rounded before a value is asked for."""
import fractions

import numpy as np


def _sorted_rows(y, p):
    p = np.asarray(p, np.float32).reshape(-1) + np.float32(0)                # -0.0 + 0.0 = +0.0: one score
    y = (np.asarray(y).reshape(-1) != 0).astype(np.int64)
    if not np.isfinite(p).all():
        raise ValueError("scores must be finite")
    o = np.lexsort((y, p))
    return y[o], p[o]


def isotonic_rows(y, p):
    """The hull form: the block ends are the vertices of the lower convex hull of (cumulative rows, cumulative positives) at the
    ends of the tie groups, from (0, 0); collinear points are no vertices."""
    y, p = _sorted_rows(y, p)
    if p.size == 0:
        return []
    ends = np.flatnonzero(np.r_[p[1:] != p[:-1], True])
    cnt = (ends + 1).tolist()
    pos = np.cumsum(y)[ends].tolist()
    hx, hy = [0], [0]
    for cx, cy in zip(cnt, pos):
        while len(hx) >= 2 and (hy[-1] - hy[-2]) * (cx - hx[-1]) >= (cy - hy[-1]) * (hx[-1] - hx[-2]):
            hx.pop()
            hy.pop()
        hx.append(cx)
        hy.append(cy)
    return [(p[hx[k - 1]], p[hx[k] - 1], hx[k] - hx[k - 1], hy[k] - hy[k - 1]) for k in range(1, len(hx))]


def isotonic_rows_slow(y, p):
    """Textbook pool-adjacent-violators, one row at a time with exact fractions; rows of one score are pooled first, and a block
    whose mean does not exceed its left neighbour's is pooled with it (equal means are one block)."""
    y, p = _sorted_rows(y, p)
    blocks = []                                                               # [x_lo, x_hi, count, positives]
    for yi, pi in zip(y.tolist(), p):
        if blocks and blocks[-1][1] == pi:
            blocks[-1][2] += 1
            blocks[-1][3] += yi
        else:
            blocks.append([pi, pi, 1, yi])
    out = []
    for b in blocks:
        out.append(list(b))
        while len(out) >= 2 and fractions.Fraction(out[-1][3], out[-1][2]) <= fractions.Fraction(out[-2][3], out[-2][2]):
            top = out.pop()
            out[-1][1] = top[1]
            out[-1][2] += top[2]
            out[-1][3] += top[3]
    return [tuple(b) for b in out]


def block_values(blocks):
    return np.array([float(np.float64(b[3]) / np.float64(b[2])) for b in blocks], np.float64)


def isotonic_apply(blocks, x, eps=0.0):
    """The map of `blocks` at the float32 scores x, float64 operations in the contract's order -> float32."""
    x = np.asarray(x, np.float32).reshape(-1).astype(np.float64)
    lo = np.array([b[0] for b in blocks], np.float32).astype(np.float64)
    hi = np.array([b[1] for b in blocks], np.float32).astype(np.float64)
    v = block_values(blocks)
    nb = len(blocks)
    k = np.clip(np.searchsorted(lo, x, side="right") - 1, 0, nb - 1)          # the largest k with lo[k] <= x
    k1 = np.minimum(k + 1, nb - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (x - hi[k]) / (lo[k1] - hi[k])
        r = v[k] + t * (v[k1] - v[k])
    r = np.where(x <= hi[k], v[k], r)
    r = np.where(x >= hi[nb - 1], v[nb - 1], r)
    r = np.where(x <= lo[0], v[0], r)
    out = r.astype(np.float32)
    if eps > 0:
        e = np.float32(eps)
        out = np.minimum(np.maximum(out, e), np.float32(1) - e)
    return out


def isotonic_exact(y, p, domain=None, n_domain=1):
    """The n_domain + 1 fits: domains 0..n_domain-1, then all rows."""
    y = np.asarray(y).reshape(-1)
    p = np.asarray(p, np.float32).reshape(-1)
    d = np.zeros(y.size, np.int64) if domain is None else np.asarray(domain).reshape(-1)
    return [isotonic_rows(y[d == s], p[d == s]) for s in range(n_domain)] + [isotonic_rows(y, p)]
