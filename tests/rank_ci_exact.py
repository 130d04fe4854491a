"""cdc_eval_rank_ci's contract as exact rationals (helper of tests/test_rank_ci_cpu.py and tests/test_gpu_rank_ci.py; not a test).

Groups, ties and the per-group values m_g are tests/rank_exact.py's (`user_runs`, `group_figures`); a group counts iff it holds a
positive.  Per segment (domain 0..n_domain-1, then ALL rows by user), figure and cut-off, over the G counted groups with weight w_g
(1, or the exact rational of the user's float weight):

    M = sum w m / sum w                var = G / (G - 1) * sum_g (w_g (m_g - M))^2 / (sum_g w_g)^2
    delta = M_a - M_b                  var_delta = G / (G - 1) * sum_g (w_g ((m_g^a - m_g^b) - delta))^2 / (sum_g w_g)^2
    M_r = sum_g w(seed, r, u_g) w_g m_g / sum_g w(seed, r, u_g) w_g         w(...) = bootstrap_exact.weights (or a stand-in)

all in fractions.Fraction.  Beside each variance stands the absolute-value sum G / (G - 1) * sum_g w_g^2 |c_g| / (sum_g w_g)^2 of its
centred values c_g (m_g - M, or (m_g^a - m_g^b) - delta), which a rounding-error bound on the variance needs.

Groups are pooled by their run signature (under both vectors when there are two): a signature's values are formed once, and per
signature only sum w, sum w^2 and the replicates' sum w(r) w are kept, so 70 000 rows take seconds.
"""
import itertools
from fractions import Fraction

import numpy as np

import bootstrap_exact
from rank_exact import FIGURES, exact_table, group_figures, user_runs


def _straddles(runs, ks):
    edges = itertools.accumulate(t for t, _ in runs)
    return any(b - t < K < b for (t, _), b in zip(runs, edges) for K in ks)


def _flat(figs):
    """{figure: [per K]} -> the values in (figure, K) order"""
    return [v for f in FIGURES for v in figs[f]]


def _shape(flat, n_k):
    return [list(flat[f * n_k:(f + 1) * n_k]) for f in range(len(FIGURES))]


def _moments(pools, vals, den, G):
    """pools: [(sum w, sum w^2)], vals: per pool the flat values -> (M, var, abs) as flat lists; var and abs None when G < 2"""
    nv = len(vals[0])
    M = [sum((p[0] * v[j] for p, v in zip(pools, vals)), Fraction(0)) / den for j in range(nv)]
    if G < 2:
        return M, None, None
    scale = Fraction(G, G - 1) / (den * den)
    var = [scale * sum((p[1] * (v[j] - M[j]) ** 2 for p, v in zip(pools, vals)), Fraction(0)) for j in range(nv)]
    ab = [scale * sum((p[1] * abs(v[j] - M[j]) for p, v in zip(pools, vals)), Fraction(0)) for j in range(nv)]
    return M, var, ab


def rank_ci_rows(y, s, u, ks, D, weights=None, s_b=None, n_rep=0, seed=0, weight_fn=bootstrap_exact.weights, memo=None):
    """One segment's rows -> a dict: G, left_out, notes, and [figure][K] lists of Fractions M, var, var_abs (with s_b also M_b, var_b,
    var_b_abs, delta, var_delta, var_delta_abs), reps / reps_b [replicate] of such lists and rep_counted [replicate].  M (M_b, delta)
    is None when G == 0, a variance (and its absolute sum) when G < 2, a replicate when no counted group has a positive weight.
    notes: straddle / straddle_b = counted groups with a tie run across some K under s / s_b."""
    memo = {} if memo is None else memo
    n_k, paired = len(ks), s_b is not None
    out = {"G": 0, "left_out": 0, "notes": {"straddle": 0, "straddle_b": 0}}
    names = ["M", "var", "var_abs"] + (["M_b", "var_b", "var_b_abs", "delta", "var_delta", "var_delta_abs"] if paired else [])
    out.update({k: None for k in names})
    out["reps"] = [None] * n_rep if n_rep else None
    out["reps_b"] = [None] * n_rep if n_rep and paired else None
    out["rep_counted"] = [0] * n_rep if n_rep else None
    if len(y) == 0:
        return out
    runs_a = user_runs(y, s, u)
    runs_b = dict(user_runs(y, s_b, u)) if paired else None
    uids = np.array([uid for uid, _ in runs_a], dtype=np.int64)
    rep_w = [np.asarray(weight_fn(seed, r, uids)).tolist() for r in range(n_rep)]
    pools = {}                                                  # signature -> [sum w, sum w^2, [sum w(r) w per replicate]]
    for pos, (uid, ra) in enumerate(runs_a):
        if not any(p for _, p in ra):
            out["left_out"] += 1
            continue
        out["G"] += 1
        sig = (ra, runs_b[uid]) if paired else (ra,)
        for r in sig:
            if r not in memo:
                memo[r] = (_flat(group_figures(r, ks, D)), _straddles(r, ks))
        out["notes"]["straddle"] += memo[ra][1]
        if paired:
            out["notes"]["straddle_b"] += memo[sig[1]][1]
        w = Fraction(1) if weights is None else Fraction(float(weights[uid]))
        p = pools.setdefault(sig, [Fraction(0), Fraction(0), [Fraction(0)] * n_rep])
        p[0] += w
        p[1] += w * w
        for r in range(n_rep):
            if rep_w[r][pos]:
                p[2][r] += rep_w[r][pos] * w
                out["rep_counted"][r] += 1
    G = out["G"]
    if G == 0:
        return out
    sigs = list(pools)
    pl = [pools[k] for k in sigs]
    den = sum((p[0] for p in pl), Fraction(0))
    va = [memo[k[0]][0] for k in sigs]
    M, var, ab = _moments(pl, va, den, G)
    out.update({"M": _shape(M, n_k), "var": var and _shape(var, n_k), "var_abs": ab and _shape(ab, n_k)})
    vecs = [("reps", va)]
    if paired:
        vb = [memo[k[1]][0] for k in sigs]
        M_b, var_b, ab_b = _moments(pl, vb, den, G)
        # the centred differences (m_a - m_b) - delta are the differences' own centred values: their mean under w is delta
        delta, var_d, ab_d = _moments(pl, [[a - b for a, b in zip(x, z)] for x, z in zip(va, vb)], den, G)
        assert delta == [a - b for a, b in zip(M, M_b)]
        out.update({"M_b": _shape(M_b, n_k), "var_b": var_b and _shape(var_b, n_k), "var_b_abs": ab_b and _shape(ab_b, n_k),
                    "delta": _shape(delta, n_k), "var_delta": var_d and _shape(var_d, n_k), "var_delta_abs": ab_d and _shape(ab_d, n_k)})
        vecs.append(("reps_b", vb))
    for r in range(n_rep):
        den_r = sum((p[2][r] for p in pl), Fraction(0))
        if out["rep_counted"][r] == 0:
            continue
        for name, vals in vecs:
            flat = [sum((p[2][r] * v[j] for p, v in zip(pl, vals)), Fraction(0)) / den_r for j in range(len(vals[0]))]
            out[name][r] = _shape(flat, n_k)
    return out


def rank_ci_exact(y, s, u, domain=None, n_domain=1, ks=(10,), D=None, weights=None, s_b=None, n_rep=0, seed=0,
                  weight_fn=bootstrap_exact.weights):
    """Every output of cdc_eval_rank_ci: a list with one `rank_ci_rows` dict per segment — domains 0..n_domain-1, then ALL rows grouped
    by user across domains.  D: the float64 discount table the device reads (at least ks[-1] + 1 entries)."""
    y, s, u = np.asarray(y), np.asarray(s), np.asarray(u)
    s_b = None if s_b is None else np.asarray(s_b)
    D = exact_table(D)
    assert len(D) > ks[-1]
    memo, out = {}, []
    for d in range(n_domain + 1):
        if d == n_domain or domain is None:
            mk = np.ones(len(y), dtype=bool)
        else:
            mk = np.asarray(domain) == d
        out.append(rank_ci_rows(y[mk], s[mk], u[mk], ks, D, weights, None if s_b is None else s_b[mk], n_rep, seed, weight_fn, memo))
    return out
