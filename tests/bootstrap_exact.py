"""The contract of cdc_eval_bootstrap without a device (helper of tests/test_bootstrap_cpu.py and tests/test_gpu_bootstrap.py; not
a test).

Weights, all arithmetic mod 2^64 in Python integers:

    mix(x):  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
    h(seed, r, c) = mix(mix(seed + 0x9E3779B97F4A7C15 (r + 1)) + c)        u = h >> 32
    w(seed, r, c) = #{k < 12 : u >= T[k]}        T[k] = floor(2^32 e^-1 sum_{j <= k} 1/j!)   (decimal, 60 digits)

a Poisson(1) variate capped at 12, one per (replicate, cluster), applied to every row of the cluster.  Per replicate r and segment
(domain 0..n_domain-1, then ALL rows), with w_i the weight of row i's cluster:

    auc   U2 / (2 Wp Wn), U2 = sum over (positive i, negative j) of w_i w_j (2 [s_j < s_i] + [s_j = s_i]), Wp = sum w_i y_i,
          Wn = W - Wp; a Fraction, None when Wp or Wn is 0
    loss  fsum(w_i l_i) / W with loss_ci_exact's per-row terms l_i; None under the same condition
    gauc  sum_g w_g omega_g A_g / sum_g w_g omega_g over the users with both classes in the segment (gauc_exact.user_sums: A_g =
          U2_g / (2 P_g N_g), omega_g = the user's rows there or user_weight[g]); a Fraction, None when no such user has w_g > 0

Two independent forms: `bootstrap_brute` counts the weighted pairs one by one, `bootstrap_sorted` takes them from one sort per
segment with int64 sums over its tie runs.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

from gauc_exact import user_sums
from loss_ci_exact import loss_terms

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_W = 12


def thresholds():
    """T[k] = floor(2^32 e^-1 sum_{j <= k} 1/j!), k < 12, from 60-digit decimals"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        inv_e = 1 / decimal.Decimal(1).exp()
        cum, out = decimal.Decimal(0), []
        for k in range(MAX_W):
            cum += 1 / decimal.Decimal(math.factorial(k))
            out.append(int((decimal.Decimal(1 << 32) * inv_e * cum).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    return out


T = thresholds()


def mix(x):
    x &= MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def weight(seed, r, c):
    u = mix(mix(seed + GOLDEN * (r + 1)) + c) >> 32
    return sum(1 for t in T if u >= t)


def weights(seed, r, clusters):
    """the weights of an array of cluster ids in replicate r -> int64 array (numpy uint64 arithmetic wraps mod 2^64; held to
    `weight` by tests/test_bootstrap_cpu.py)"""
    x = (np.asarray(clusters).astype(np.uint64) + np.uint64(mix(seed + GOLDEN * (r + 1)))).astype(np.uint64)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    u = (x >> np.uint64(32)).astype(np.int64)
    return (u[:, None] >= np.asarray(T, dtype=np.int64)[None, :]).sum(1).astype(np.int64)


def ones(seed, r, clusters):
    """stands in for `weights`: every cluster once — the unweighted figures"""
    return np.ones(len(clusters), dtype=np.int64)


def _f32(s):
    return np.asarray(s, dtype=np.float32) + np.float32(0.0)               # -0.0 -> +0.0: one tie group


def _auc_brute(y, s, w):
    pos = [(float(a), int(b)) for a, b, c in zip(s, w, y) if c and b]
    neg = [(float(a), int(b)) for a, b, c in zip(s, w, y) if not c and b]
    u2 = 0
    for si, wi in pos:
        for sj, wj in neg:
            u2 += wi * wj * (2 if sj < si else (1 if sj == si else 0))
    return u2


def _auc_sorted(y, s, w):
    """U2 from one sort: a tie run's weighted positives meet twice the weighted negatives below the run and once those inside it"""
    if len(y) == 0:
        return 0
    order = np.argsort(s, kind="stable")
    y, s, w = y[order], s[order], w[order]
    new = np.r_[True, s[1:] != s[:-1]]
    run = np.cumsum(new) - 1
    wp_run = np.zeros(run[-1] + 1, dtype=np.int64)
    wn_run = np.zeros(run[-1] + 1, dtype=np.int64)
    np.add.at(wp_run, run, w * y)
    np.add.at(wn_run, run, w * (1 - y))
    below = np.cumsum(wn_run) - wn_run
    return sum(int(p) * (2 * int(b) + int(m)) for p, b, m in zip(wp_run, below, wn_run))


def _gauc(y, s, u, wg_of, user_weight):
    """-> (Fraction or None, users counted: both classes in these rows)"""
    if len(y) == 0:
        return None, 0
    uid, U2, P, N = user_sums(y, s, u)
    ok = (P > 0) & (N > 0)
    K = int(ok.sum())
    num = den = Fraction(0)
    live = 0
    for g, u2, p, m in zip(uid[ok].tolist(), U2[ok].tolist(), P[ok].tolist(), N[ok].tolist()):
        wg = wg_of(g)
        if wg == 0:
            continue
        live += 1
        omega = Fraction(p + m) if user_weight is None else Fraction(float(user_weight[g]))
        num += wg * omega * Fraction(u2, 2 * p * m)
        den += wg * omega
    return (num / den if live else None), K


def _bootstrap(auc_u2, y, s, cluster, seed, n_rep, domain, n_domain, user_weight, gauc, weight_fn):
    y = (np.asarray(y) != 0).astype(np.int64)
    s = _f32(s)
    n = len(y)
    row_clusters = cluster is None
    c = np.arange(n, dtype=np.int64) if row_clusters else np.asarray(cluster).astype(np.int64)
    if gauc is None:
        gauc = not row_clusters
    terms = np.array(loss_terms(y, s), dtype=np.float64)
    masks = [np.ones(n, dtype=bool) if d == n_domain or domain is None else np.asarray(domain) == d for d in range(n_domain + 1)]
    out = []
    for r in range(n_rep):
        w = np.asarray(weight_fn(seed, r, c), dtype=np.int64)
        wg = dict(zip(c.tolist(), w.tolist()))
        segs = []
        for mk in masks:
            ys, ss, ws = y[mk], s[mk], w[mk]
            W, Wp = int(ws.sum()), int((ws * ys).sum())
            e = {"W": W, "Wp": Wp, "rows": int(mk.sum()), "auc": None, "loss": None, "terms": None, "gauc": None, "K": 0}
            if Wp > 0 and W - Wp > 0:
                e["auc"] = Fraction(auc_u2(ys, ss, ws), 2 * Wp * (W - Wp))
                e["terms"] = [float(a) * float(b) for a, b in zip(ws.tolist(), terms[mk].tolist()) if a]
                e["loss"] = math.fsum(e["terms"]) / W
            if gauc:
                e["gauc"], e["K"] = _gauc(ys, ss, c[mk], wg.__getitem__, user_weight)
            segs.append(e)
        out.append(segs)
    return out


def bootstrap_brute(y, s, cluster=None, seed=0, n_rep=1, domain=None, n_domain=1, user_weight=None, gauc=None, weight_fn=weights):
    """-> [replicate][segment] dict(W, Wp, rows, auc, loss, terms, gauc, K); the weighted (positive, negative) pairs one by one"""
    return _bootstrap(_auc_brute, y, s, cluster, seed, n_rep, domain, n_domain, user_weight, gauc, weight_fn)


def bootstrap_sorted(y, s, cluster=None, seed=0, n_rep=1, domain=None, n_domain=1, user_weight=None, gauc=None, weight_fn=weights):
    """as bootstrap_brute, the pair counts from one sort per segment: O(n log n), for the chunk-sized cases"""
    return _bootstrap(_auc_sorted, y, s, cluster, seed, n_rep, domain, n_domain, user_weight, gauc, weight_fn)


def as_float(v):
    return float("nan") if v is None else float(v)
