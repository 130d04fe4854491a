"""The per-user top-K figures as exact rationals (helper of tests/test_rank_cpu.py and tests/test_gpu_rank.py; not a test).

cdc_eval_rank's contract restated without floating point.  A group (a user's rows) is ranked by descending score, -0.0 and +0.0
being one score; its tie runs t occupy the 0-based ranks [a_t, b_t) with T_t rows of which P_t are positive, and every figure is
the expectation over a uniformly random order of the tied rows (McSherry & Najork 2008), in closed form, with
c_t = max(0, min(b_t, K) - a_t) and P the group's positives:

    H         = sum_t P_t c_t / T_t            recall = H / P            precision = H / K
    ndcg      = sum_{a_t < K} (P_t / T_t) (D[min(b_t, K)] - D[a_t]) / D[min(P, K)]
    hit       = 1 - prod_{a_t < K, P_t > 0} q_t,  q_t = 0 if c_t > T_t - P_t else prod_{i < c_t} (T_t - P_t - i) / (T_t - i)
    mrr       = sum_{j=0}^{min(T - Pt, K - a - 1)} pr_j / (a + 1 + j) over the first run (a, T, Pt) with a positive, 0 if a >= K,
                pr_0 = Pt / T, pr_{j+1} = pr_j (T - Pt - j) / (T - 1 - j)

The discount table D (D[0] = 0, D[r+1] = D[r] + 1/log2(r+2)) is an ARGUMENT, and every entry is taken as the exact rational of that
double: a floating subtraction D[b] - D[a] is correctly rounded, so a device that reads the same table is held to these values
with no margin for the table itself.  A segment's value is sum_g w_g m_g / sum_g w_g over its groups with P >= 1 (w_g = 1, or the
exact rational of the user's float weight), all in fractions.Fraction.  `brute_force` enumerates every order of the tied rows of a
tiny group instead.
"""
import itertools
from fractions import Fraction

import numpy as np

FIGURES = ("ndcg", "recall", "precision", "hit", "mrr")


def exact_table(table):
    """the float64 discount table -> the exact rational of every entry"""
    return [Fraction(float(v)) for v in np.asarray(table, dtype=np.float64).tolist()]


def group_figures(runs, ks, D):
    """runs: the group's tie runs in rank order as (T_t, P_t); D: exact_table(...) -> {figure: [Fraction per K]}, the group must hold
    a positive."""
    P = sum(p for _, p in runs)
    assert P >= 1
    bounds, a = [], 0
    for T, Pt in runs:
        bounds.append((a, a + T, T, Pt))
        a += T
    out = {f: [] for f in FIGURES}
    for K in ks:
        H, dcg, miss = Fraction(0), Fraction(0), Fraction(1)
        for a, b, T, Pt in bounds:
            if a >= K:
                break
            c = min(b, K) - a
            H += Fraction(Pt * c, T)
            dcg += Fraction(Pt, T) * (D[min(b, K)] - D[a])
            if Pt > 0:
                if c > T - Pt:
                    miss = Fraction(0)
                else:
                    for i in range(c):
                        miss *= Fraction(T - Pt - i, T - i)
        mrr = Fraction(0)
        a, _, T, Pt = next(r for r in bounds if r[3] > 0)
        if a < K:
            pr = Fraction(Pt, T)
            for j in range(min(T - Pt, K - a - 1) + 1):
                mrr += pr / (a + 1 + j)
                if j < T - Pt:
                    pr *= Fraction(T - Pt - j, T - 1 - j)
        out["ndcg"].append(dcg / D[min(P, K)])
        out["recall"].append(H / P)
        out["precision"].append(H / K)
        out["hit"].append(1 - miss)
        out["mrr"].append(mrr)
    return out


def brute_force(runs, ks, D):
    """the same figures as the plain average over EVERY arrangement of the labels inside the tie runs (each arrangement stands for the
    same number of row orders): the definition the closed forms are checked against.  Tiny groups only."""
    per_run = []
    for T, Pt in runs:
        per_run.append([tuple(1 if i in pos else 0 for i in range(T)) for pos in itertools.combinations(range(T), Pt)])
    P = sum(p for _, p in runs)
    total = {f: [Fraction(0)] * len(ks) for f in FIGURES}
    count = 0
    for pick in itertools.product(*per_run):
        labels = [v for run in pick for v in run]
        count += 1
        for q, K in enumerate(ks):
            top = labels[:K]
            hits = sum(top)
            dcg = sum((D[r + 1] - D[r] for r, v in enumerate(top) if v), Fraction(0))
            first = top.index(1) if hits else None
            add = {"ndcg": dcg / D[min(P, K)], "recall": Fraction(hits, P), "precision": Fraction(hits, K),
                   "hit": Fraction(1 if hits else 0), "mrr": Fraction(1, first + 1) if hits else Fraction(0)}
            for f in FIGURES:
                total[f][q] = total[f][q] + add[f]
    return {f: [v / count for v in total[f]] for f in FIGURES}


def user_runs(y, s, u):
    """-> [(user id, ((T_t, P_t), ...) in rank order)] for every user of these rows, sorted by id"""
    y, u = np.asarray(y).astype(np.int64), np.asarray(u).astype(np.int64)
    s = np.asarray(s, dtype=np.float32) + np.float32(0.0)                  # -0.0 -> +0.0: one tie run
    n = len(y)
    order = np.lexsort((-s, u))                                            # by user, then by descending score
    y, s, u = y[order], s[order], u[order]
    new_g = np.r_[True, u[1:] != u[:-1]]
    new_t = new_g | np.r_[True, s[1:] != s[:-1]]
    t_start = np.flatnonzero(new_t)
    T = np.diff(np.r_[t_start, n])
    Pt = np.add.reduceat((y == 1).astype(np.int64), t_start)
    run_user = u[t_start]
    first_run = np.flatnonzero(new_g[t_start])
    stops = np.r_[first_run[1:], len(t_start)]
    T, Pt = T.tolist(), Pt.tolist()
    return [(int(run_user[a]), tuple(zip(T[a:b], Pt[a:b]))) for a, b in zip(first_run.tolist(), stops.tolist())]


def rank_rows(y, s, u, ks, D, weights=None):
    """The figures of one set of rows -> ({figure: [Fraction per K]} or None when no user is counted, users counted, users left out,
    notes); notes counts what a test may want its input to contain: counted groups shorter than some K, with a tie run that straddles
    some K (a_t < K < b_t), and without a negative."""
    notes = {"short": 0, "straddle": 0, "no_negative": 0}
    if len(y) == 0:
        return None, 0, 0, notes
    memo, counted, left_out = {}, 0, 0
    sums = {f: [{} for _ in ks] for f in FIGURES}                          # per denominator: few distinct ones, the sums stay small
    den = Fraction(0)
    for uid, runs in user_runs(y, s, u):
        if not any(p for _, p in runs):
            left_out += 1
            continue
        counted += 1
        if runs not in memo:
            rows = sum(t for t, _ in runs)
            edges = list(itertools.accumulate(t for t, _ in runs))
            memo[runs] = (group_figures(runs, ks, D), any(rows < K for K in ks),
                          any(b - t < K < b for (t, _), b in zip(runs, edges) for K in ks), all(t == p for t, p in runs))
        figs, short, straddle, no_neg = memo[runs]
        notes["short"] += short
        notes["straddle"] += straddle
        notes["no_negative"] += no_neg
        w = Fraction(1) if weights is None else Fraction(float(weights[uid]))
        den += w
        for f in FIGURES:
            for q, v in enumerate(figs[f]):
                v = w * v
                by_den = sums[f][q]
                by_den[v.denominator] = by_den.get(v.denominator, 0) + v.numerator
    if counted == 0:
        return None, 0, left_out, notes
    vals = {f: [sum((Fraction(v, d) for d, v in sorted(by_den.items())), Fraction(0)) / den for by_den in sums[f]] for f in FIGURES}
    return vals, counted, left_out, notes


def rank_exact(y, s, u, domain=None, n_domain=1, ks=(10,), D=None, weights=None):
    """Every figure of cdc_eval_rank: (vals, counted, left_out, notes) with one entry per segment — domains 0..n_domain-1, then ALL
    rows grouped by user across domains; vals[segment] is {figure: [Fraction per K]}, or None where no group is counted.  D: the
    float64 discount table the device reads (at least ks[-1] + 1 entries)."""
    y, s, u = np.asarray(y), np.asarray(s), np.asarray(u)
    D = exact_table(D)
    assert len(D) > ks[-1]
    vals, counted, left, notes = [], [], [], []
    for d in range(n_domain + 1):
        if d == n_domain or domain is None:
            mk = np.ones(len(y), dtype=bool)                               # n_domain == 1 without a column: the one domain is every row
        else:
            mk = np.asarray(domain) == d
        v, c, l, nt = rank_rows(y[mk], s[mk], u[mk], ks, D, weights)
        vals.append(v)
        counted.append(c)
        left.append(l)
        notes.append(nt)
    return vals, counted, left, notes
