"""DeLong's AUC variance and the paired comparison of two score vectors as exact rationals (helper of tests/test_delong_cpu.py
and tests/test_gpu_delong.py; not a test).  The contract, per segment (one domain's rows, or all rows), positives x_1..x_P,
negatives y_1..y_N, psi(x, y) = 1, 1/2, 0 for x >, =, < y with -0.0 == +0.0:

    a_i = 2 sum_j psi(x_i, y_j)      c_j = 2 sum_i psi(x_i, y_j)                                   (integers)
    auc = sum a / (2 P N)
    S10 = [P sum a^2 - (sum a)^2] / [P (P-1) 4 N^2]      S01 = [N sum c^2 - (sum c)^2] / [N (N-1) 4 P^2]
    var = S10 / P + S01 / N;   paired: delta = auc_a - auc_b, var_delta = the same on d = a - b, f = c - e

Two independent forms:
  (a) `delong_brute`: every one of the P N pairs straight from psi, the variances by the textbook definition
      S10 = sum_i (V10_i - auc)^2 / (P - 1) with V10_i = sum_j psi(x_i, y_j) / N, all in fractions.Fraction;
  (b) `delong_exact`: counts from a numpy sort (O(n log n)), the sums as Python ints (chunked so that no numpy integer
      overflows), the integer formulas above.
A value is a Fraction, or None where the contract says NaN (auc, delta: P == 0 or N == 0; a variance: P < 2 or N < 2).
"""
from fractions import Fraction

import numpy as np

CHUNK = 1 << 20


def _f32(s):
    return np.asarray(s, dtype=np.float32) + np.float32(0.0)               # -0.0 -> +0.0: one tie group


# ---------------------------------------------------------------------------------------------------------------------
# (a) brute force
# ---------------------------------------------------------------------------------------------------------------------
def _psi(x, y):
    return Fraction(1) if x > y else (Fraction(1, 2) if x == y else Fraction(0))


def _v(x, y):
    """V10 [P], V01 [N]: every positive's / negative's mean psi against the other class"""
    v10 = [sum((_psi(xi, yj) for yj in y), Fraction(0)) / len(y) for xi in x]
    v01 = [sum((_psi(xi, yj) for xi in x), Fraction(0)) / len(x) for yj in y]
    return v10, v01


def _textbook_var(v10, v01):
    P, N = len(v10), len(v01)
    if P < 2 or N < 2:
        return None
    m10, m01 = sum(v10, Fraction(0)) / P, sum(v01, Fraction(0)) / N
    s10 = sum(((v - m10) ** 2 for v in v10), Fraction(0)) / (P - 1)
    s01 = sum(((v - m01) ** 2 for v in v01), Fraction(0)) / (N - 1)
    return s10 / P + s01 / N


def delong_brute(y, s, s_b=None):
    """One set of rows -> dict(auc, var[, auc_b, var_b, delta, var_delta])"""
    y = np.asarray(y)
    s = _f32(s)
    pos, neg = np.flatnonzero(y != 0), np.flatnonzero(y == 0)
    P, N = len(pos), len(neg)
    if P == 0 or N == 0:
        r = {"auc": None, "var": None}
        if s_b is not None:
            r.update({"auc_b": None, "var_b": None, "delta": None, "var_delta": None})
        return r
    v10, v01 = _v([float(v) for v in s[pos]], [float(v) for v in s[neg]])
    r = {"auc": sum(v10, Fraction(0)) / P, "var": _textbook_var(v10, v01)}
    if s_b is not None:
        sb = _f32(s_b)
        w10, w01 = _v([float(v) for v in sb[pos]], [float(v) for v in sb[neg]])
        r["auc_b"], r["var_b"] = sum(w10, Fraction(0)) / P, _textbook_var(w10, w01)
        r["delta"] = r["auc"] - r["auc_b"]
        r["var_delta"] = _textbook_var([p - q for p, q in zip(v10, w10)], [p - q for p, q in zip(v01, w01)])
    return r


# ---------------------------------------------------------------------------------------------------------------------
# (b) sort and mid-rank counts
# ---------------------------------------------------------------------------------------------------------------------
def placements(y, s):
    """-> (a int64 [P] in the order of the positive rows, c int64 [N] in the order of the negative rows)"""
    y = np.asarray(y) != 0
    s = _f32(s)
    _, inv = np.unique(s, return_inverse=True)                             # ascending distinct scores
    inv = inv.reshape(-1)
    k = int(inv.max()) + 1 if len(inv) else 0
    n_pos = np.bincount(inv[y], minlength=k).astype(np.int64)
    n_neg = np.bincount(inv[~y], minlength=k).astype(np.int64)
    neg_below = np.cumsum(n_neg) - n_neg
    pos_above = n_pos.sum() - np.cumsum(n_pos)
    a = (2 * neg_below + n_neg)[inv[y]]
    c = (2 * pos_above + n_pos)[inv[~y]]
    return a, c


def int_sum(x):
    """sum of an int64 array with |x| < 2^32 as a Python int"""
    return sum(int(x[i:i + CHUNK].sum()) for i in range(0, len(x), CHUNK))


def int_sum_sq(x):
    """sum of squares of an int64 array with |x| < 2^32 as a Python int: 16-bit halves, a chunk's partial sums stay below 2^52"""
    x = np.abs(x)
    total = 0
    for i in range(0, len(x), CHUNK):
        hi, lo = x[i:i + CHUNK] >> 16, x[i:i + CHUNK] & 0xffff
        total += (int((hi * hi).sum()) << 32) + (int((hi * lo).sum()) << 17) + int((lo * lo).sum())
    return total


def _var(P, N, p1, p2, n1, n2):
    if P < 2 or N < 2:
        return None
    s10 = Fraction(P * p2 - p1 * p1, P * (P - 1) * 4 * N * N)
    s01 = Fraction(N * n2 - n1 * n1, N * (N - 1) * 4 * P * P)
    return s10 / P + s01 / N


def delong_rows(y, s, s_b=None):
    """One set of rows -> dict(rows, P, N, auc, var, sums=(sum a, sum a^2, sum c, sum c^2)[, auc_b, var_b, delta, var_delta])"""
    y = np.asarray(y)
    P = int((y != 0).sum())
    N = len(y) - P
    a, c = placements(y, s)
    sums = (int_sum(a), int_sum_sq(a), int_sum(c), int_sum_sq(c))
    both = P > 0 and N > 0
    r = {"rows": len(y), "P": P, "N": N, "sums": sums, "auc": Fraction(sums[0], 2 * P * N) if both else None, "var": _var(P, N, *sums)}
    if s_b is not None:
        b, e = placements(y, s_b)
        sb = (int_sum(b), int_sum_sq(b), int_sum(e), int_sum_sq(e))
        d, f = a - b, c - e
        r["auc_b"], r["var_b"] = (Fraction(sb[0], 2 * P * N) if both else None), _var(P, N, *sb)
        r["delta"] = Fraction(int_sum(d), 2 * P * N) if both else None
        r["var_delta"] = _var(P, N, int_sum(d), int_sum_sq(d), int_sum(f), int_sum_sq(f))
    return r


def delong_exact(y, s, s_b=None, domain=None, n_domain=1):
    """Every figure of cdc_eval_auc_delong: a list with n_domain + 1 entries (domains 0..n_domain-1, then ALL rows) of delong_rows'
    dictionaries."""
    y, s = np.asarray(y), np.asarray(s)
    s_b = None if s_b is None else np.asarray(s_b)
    everything = delong_rows(y, s, s_b)
    if domain is None:                                                     # n_domain == 1: the one domain is every row
        return [everything] * (n_domain + 1)
    out = []
    for d in range(n_domain):
        mk = np.asarray(domain) == d
        out.append(delong_rows(y[mk], s[mk], None if s_b is None else s_b[mk]))
    return out + [everything]


def as_float(v):
    return float("nan") if v is None else float(v)
