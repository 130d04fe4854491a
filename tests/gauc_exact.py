"""GAUC as an exact rational (helper of tests/test_gauc_cpu.py and tests/test_gpu_gauc.py; not a test).

The reference's gauc_score (base.py:33-64) restated without floating point: rows are sorted by (user, score) once per
(pseudo-)domain, every positive row's twice-mid-rank inside its user's run comes from the run and tie boundaries of that sort,
and the per-user sums S2, P, rows are integer reduceat's.  With U2 = S2 - P(P+1) = twice the Mann-Whitney U,

    GAUC = sum_g w_g * U2_g / (2 P_g N_g)  /  sum_g w_g        over the users g with P_g > 0 and N_g > 0,

is formed in fractions.Fraction (a float weight is the exact rational it stands for), so the value carries no rounding at all
and float() of it is the correctly rounded double.
"""
from fractions import Fraction

import numpy as np


def user_sums(y, s, u):
    """-> (user ids present, U2, P, N) as int64 arrays, one entry per user of these rows (sorted by id)."""
    y, u = np.asarray(y).astype(np.int64), np.asarray(u).astype(np.int64)
    s = np.asarray(s, dtype=np.float32) + np.float32(0.0)                  # -0.0 -> +0.0: one tie group
    n = len(y)
    order = np.lexsort((s, u))                                             # by user, then by score
    y, s, u = y[order], s[order], u[order]
    new_g = np.r_[True, u[1:] != u[:-1]]
    new_t = new_g | np.r_[True, s[1:] != s[:-1]]
    g_start, t_start = np.flatnonzero(new_g), np.flatnonzero(new_t)
    t_end = np.r_[t_start[1:], n] - 1
    run_of, grp_of = np.cumsum(new_t) - 1, np.cumsum(new_g) - 1
    h = g_start[grp_of]
    twice_midrank = (t_start[run_of] - h) + (t_end[run_of] - h) + 2        # 0-based first + last position -> twice the 1-based mid-rank
    S2 = np.add.reduceat(np.where(y == 1, twice_midrank, 0).astype(np.int64), g_start)
    P = np.add.reduceat((y == 1).astype(np.int64), g_start)
    rows = np.diff(np.r_[g_start, n])
    return u[g_start], S2 - P * (P + 1), P, rows - P


def gauc_rows(y, s, u, weights=None):
    """GAUC of one set of rows -> (Fraction or None when no user is counted, users counted, users left out)."""
    if len(y) == 0:
        return None, 0, 0
    uid, U2, P, N = user_sums(y, s, u)
    ok = (P > 0) & (N > 0)
    counted, left_out = int(ok.sum()), int((~ok).sum())
    if counted == 0:
        return None, 0, left_out
    uid, U2, den = uid[ok], U2[ok], 2 * P[ok] * N[ok]
    if weights is None:
        w = [int(v) for v in (P + N)[ok]]
    else:
        w = [Fraction(float(weights[int(k)])) for k in uid]
        scale = 1
        for v in w:
            scale = max(scale, v.denominator)                              # denominators are powers of two
        w = [int(v * scale) for v in w]
    by_den = {}                                                            # few distinct denominators: the sum stays small
    for wi, u2, d in zip(w, U2.tolist(), den.tolist()):
        by_den[d] = by_den.get(d, 0) + wi * u2
    num = sum((Fraction(v, d) for d, v in sorted(by_den.items())), Fraction(0))
    return num / sum(w), counted, left_out


def gauc_exact(y, s, u, domain=None, n_domain=1, weights=None):
    """Every figure of cdc_eval_gauc: lists with n_domain + 1 entries (domains 0..n_domain-1, then ALL rows grouped by user across
    domains) of the value (Fraction, or None where no group is counted), the groups counted and the groups left out."""
    y, s, u = np.asarray(y), np.asarray(s), np.asarray(u)
    vals, counted, left = [], [], []
    for d in range(n_domain + 1):
        if d == n_domain:
            mk = np.ones(len(y), dtype=bool)
        elif domain is None:
            mk = np.ones(len(y), dtype=bool)                               # n_domain == 1: the one domain is every row
        else:
            mk = np.asarray(domain) == d
        v, c, l = gauc_rows(y[mk], s[mk], u[mk], weights)
        vals.append(v)
        counted.append(c)
        left.append(l)
    return vals, counted, left


def as_float(v):
    return float("nan") if v is None else float(v)
