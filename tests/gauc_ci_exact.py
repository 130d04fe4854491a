"""GAUC with its user-clustered variance as exact rationals (helper of tests/test_eval_ci_cpu.py and tests/test_gpu_eval_ci.py; not
a test).

Over the K counted users g of a set of rows (both classes present), with weight w_g (the user's row count, or a given float taken
as the exact rational it stands for) and AUC A_g:

    G = sum w A / sum w        var = K / (K - 1) * sum (w_g (A_g - G))^2 / (sum w)^2

and with a second score vector (AUCs B_g):  delta = G_a - G_b,  var_delta = the same formula on (A_g - B_g) - delta.  Two
independent forms, both in fractions.Fraction:
  gauc_ci_brute   every user's AUC by counting its (positive, negative) pairs one by one, and the textbook sum of squares
  gauc_ci_rows    from gauc_exact.user_sums (rank sums of one sort), with the moment expansion
                  sum (w (A - G))^2 = sum w^2 A^2 - 2 G sum w^2 A + G^2 sum w^2, the sums grouped by the few distinct denominators
G is None when K == 0, a variance when K < 2.
"""
import math
from fractions import Fraction

import numpy as np

from gauc_exact import user_sums


def _weights(uid, rows, weights):
    """-> integer weights (float weights scaled by a common power of two: every figure is a ratio that the scale leaves alone)"""
    if weights is None:
        return [int(v) for v in rows]
    w = [Fraction(float(weights[int(k)])) for k in uid]
    scale = 1
    for v in w:
        scale = max(scale, v.denominator)                                  # denominators are powers of two
    return [int(v * scale) for v in w]


def _pair_auc(ys, ss):
    pos = [float(v) for v, t in zip(ss, ys) if t]
    neg = [float(v) for v, t in zip(ss, ys) if not t]
    if not pos or not neg:
        return None
    twice = sum(2 * (p > q) + (p == q) for p in pos for q in neg)          # -0.0 == 0.0: a tie
    return Fraction(twice, 2 * len(pos) * len(neg))


def gauc_ci_brute(y, s, u, weights=None, sb=None):
    """Form (a).  -> dict: gauc, var, counted, left_out (and gauc_b, var_b, delta, var_delta with sb)."""
    y, u = np.asarray(y).astype(np.int64), np.asarray(u).astype(np.int64)
    s = np.asarray(s, dtype=np.float32)
    sb = None if sb is None else np.asarray(sb, dtype=np.float32)
    A, B, uid, rows, left = [], [], [], [], 0
    for k in sorted(set(u.tolist())):
        mk = u == k
        a = _pair_auc(y[mk], s[mk])
        if a is None:
            left += 1
            continue
        A.append(a)
        B.append(None if sb is None else _pair_auc(y[mk], sb[mk]))
        uid.append(k)
        rows.append(int(mk.sum()))
    K = len(A)
    keys = ("gauc", "var") + (("gauc_b", "var_b", "delta", "var_delta") if sb is not None else ())
    r = {"counted": K, "left_out": left, **{k: None for k in keys}}
    if K == 0:
        return r
    w = _weights(uid, rows, weights)
    W = sum(w)

    def ratio(v):
        return sum(wi * vi for wi, vi in zip(w, v)) / W

    def var(v, centre):
        return Fraction(K, K - 1) * sum((wi * (vi - centre)) ** 2 for wi, vi in zip(w, v)) / W ** 2 if K >= 2 else None

    r["gauc"] = ratio(A)
    r["var"] = var(A, r["gauc"])
    if sb is not None:
        r["gauc_b"] = ratio(B)
        r["var_b"] = var(B, r["gauc_b"])
        r["delta"] = r["gauc"] - r["gauc_b"]
        r["var_delta"] = var([a - b for a, b in zip(A, B)], r["delta"])
    return r


def _moments(w, num, den):
    """-> (sum w v, sum w^2 v, sum w^2 v^2) for v = num / den, as Fractions: integer sums per distinct denominator, brought onto the
    denominators' least common multiple once"""
    by = {}
    for wi, x, d in zip(w, num, den):
        t = by.setdefault(d, [0, 0, 0])
        t[0] += wi * x
        t[1] += wi * wi * x
        t[2] += wi * wi * x * x
    lcm = 1
    for d in by:
        lcm = lcm * d // math.gcd(lcm, d)
    s1 = Fraction(sum(t[0] * (lcm // d) for d, t in by.items()), lcm)
    m1 = Fraction(sum(t[1] * (lcm // d) for d, t in by.items()), lcm)
    m2 = Fraction(sum(t[2] * (lcm // d) ** 2 for d, t in by.items()), lcm * lcm)
    return s1, m1, m2


def gauc_ci_rows(y, s, u, weights=None, sb=None):
    """Form (b).  gauc_ci_brute's dict, and for the bounds of the device test the float "abs" = K / (K - 1) sum w^2 |A - G|
    (|A| + |G|) / (sum w)^2 (with sb also "abs_b", and "abs_delta" = K / (K - 1) sum w^2 |A - B - delta| (|A| + |B| + |G_a| + |G_b|) /
    (sum w)^2): what a rounding error of A, B and G is multiplied by on its way into a variance."""
    keys = ("gauc", "var") + (("gauc_b", "var_b", "delta", "var_delta") if sb is not None else ())
    r = {"counted": 0, "left_out": 0, **{k: None for k in keys}}
    if len(y) == 0:
        return r
    uid, U2, P, N = user_sums(y, s, u)
    ok = (P > 0) & (N > 0)
    K = int(ok.sum())
    r["counted"], r["left_out"] = K, int((~ok).sum())
    if K == 0:
        return r
    w = _weights(uid[ok], (P + N)[ok], weights)
    den = (2 * P * N)[ok].tolist()
    W, M0 = sum(w), sum(v * v for v in w)
    wf = np.array([float(v) for v in w]) / float(W)
    scale = Fraction(K, K - 1) / W ** 2 if K >= 2 else None
    fscale = K / (K - 1) if K >= 2 else float("nan")

    def figures(num):
        s1, m1, m2 = _moments(w, num, den)
        return s1 / W, m1, m2

    ua = U2[ok].tolist()
    G, m1, m2 = figures(ua)
    r["gauc"] = G
    Af = np.array(ua, dtype=np.float64) / np.array(den, dtype=np.float64)
    if K >= 2:
        r["var"] = scale * (m2 - 2 * G * m1 + G * G * M0)
        r["abs"] = fscale * float(np.sum(wf * wf * np.abs(Af - float(G)) * (np.abs(Af) + abs(float(G)))))
    if sb is not None:
        uid_b, U2b, Pb, Nb = user_sums(y, sb, u)
        assert np.array_equal(uid, uid_b) and np.array_equal(P, Pb) and np.array_equal(N, Nb)
        ub = U2b[ok].tolist()
        Gb, m1, m2 = figures(ub)
        r["gauc_b"] = Gb
        delta = G - Gb
        r["delta"] = delta
        Bf = np.array(ub, dtype=np.float64) / np.array(den, dtype=np.float64)
        if K >= 2:
            r["var_b"] = scale * (m2 - 2 * Gb * m1 + Gb * Gb * M0)
            r["abs_b"] = fscale * float(np.sum(wf * wf * np.abs(Bf - float(Gb)) * (np.abs(Bf) + abs(float(Gb)))))
            ud = [a - b for a, b in zip(ua, ub)]
            _, m1, m2 = figures(ud)
            r["var_delta"] = scale * (m2 - 2 * delta * m1 + delta * delta * M0)
            Df = np.array(ud, dtype=np.float64) / np.array(den, dtype=np.float64)
            r["abs_delta"] = fscale * float(np.sum(wf * wf * np.abs(Df - float(delta)) * (np.abs(Af) + np.abs(Bf) + abs(float(G)) + abs(float(Gb)))))
    return r


def gauc_ci_exact(y, s, u, domain=None, n_domain=1, weights=None, sb=None, rows=gauc_ci_rows):
    """Every figure of cdc_eval_gauc_ci: a list with n_domain + 1 entries (domains 0..n_domain-1, then ALL rows grouped by user
    across domains) of the dicts of `rows` (gauc_ci_rows or gauc_ci_brute)."""
    y, s, u = np.asarray(y), np.asarray(s), np.asarray(u)
    sb = None if sb is None else np.asarray(sb)
    out = []
    for d in range(n_domain + 1):
        mk = np.ones(len(y), dtype=bool) if d == n_domain or domain is None else np.asarray(domain) == d
        out.append(rows(y[mk], s[mk], u[mk], weights, None if sb is None else sb[mk]))
    return out


def as_float(v):
    return float("nan") if v is None else float(v)
