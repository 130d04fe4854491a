"""Times eval_rank beside eval_gauc on the same evaluation set, in the same run, and beside the route through the host (the
predictions copied back, the same five figures with the same tie expectation in numpy): 500 000 rows, 50 000 Zipf-distributed users,
3 and 50 domains, ks = (1, 5, 10, 50) by default — the evaluation set of tools/eval_ci_bench.py.

eval_gauc is the yardstick because eval_rank runs its keys, sort and first scan, skips the second scan and walks every group's head
where eval_gauc takes two differences per group.  The two device calls alternate, 20 repetitions after a warm-up, each repetition
between two device events (workspace allocation from the caching allocator included, as a caller pays it); the numpy route is timed
once, the copies to the host included.  Needs a GPU: there is no fallback.  Prints one JSON line per domain count, with the largest
difference between the device's and numpy's figures; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import RANK_FIGURES, eval_gauc, eval_rank, rank_discounts  # noqa: E402


def numpy_rank(pred, label, user, domain, n_domain, ks):
    """the figures of eval_rank through the host -> [5, len(ks), n_domain + 1]: one lexsort per segment, the tie runs by reduceat,
    hit and mrr from the first run with a positive in a loop over the ranks of that run, vectorised over the groups"""
    s_all, y_all = pred.cpu().numpy() + np.float32(0), label.cpu().numpy().astype(np.int64)
    u_all, d_all = user.cpu().numpy().astype(np.int64), domain.cpu().numpy()
    D = rank_discounts(ks[-1]).numpy()
    out = np.full((len(RANK_FIGURES), len(ks), n_domain + 1), np.nan)
    for seg in range(n_domain + 1):
        mk = slice(None) if seg == n_domain else d_all == seg
        y, u, s = y_all[mk], u_all[mk], s_all[mk]
        n = y.size
        if n == 0:
            continue
        order = np.lexsort((-s, u))
        y, u, s = y[order], u[order], s[order]
        new_g = np.r_[True, u[1:] != u[:-1]]
        new_t = new_g | np.r_[True, s[1:] != s[:-1]]
        g_start, t_start = np.flatnonzero(new_g), np.flatnonzero(new_t)
        T = np.diff(np.r_[t_start, n])
        Pt = np.add.reduceat(y, t_start)
        grp_of_run = np.cumsum(new_g)[t_start] - 1
        a = t_start - g_start[grp_of_run]
        b = a + T
        run0 = np.flatnonzero(new_g[t_start])                           # the first run of every group
        P = np.add.reduceat(Pt, run0)
        ok = P > 0
        if not ok.any():
            continue
        first = np.minimum.reduceat(np.where(Pt > 0, np.arange(T.size), T.size), run0)[ok]   # the first run with a positive
        fa, fT, fP = a[first], T[first].astype(np.float64), Pt[first].astype(np.float64)
        fN = fT - fP
        Pk = P[ok]
        for q, K in enumerate(ks):
            c = np.clip(np.minimum(b, K) - a, 0, None)
            H = np.add.reduceat(Pt * c / T, run0)[ok]
            dcg = np.add.reduceat(Pt / T * (D[np.minimum(b, K)] - D[np.minimum(a, K)]), run0)[ok]
            fc = np.clip(np.minimum(fa + fT, K) - fa, 0, None)
            miss, pr, rr = np.ones(first.size), fP / fT, np.zeros(first.size)
            for j in range(int(fc.max())):
                live = (j < fc) & (j <= fN)
                rr += np.where(live, pr / (fa + 1 + j), 0.0)
                miss *= np.where(live, (fN - j) / np.maximum(fT - j, 1), 1.0)
                pr *= np.where(live & (j < fN), (fN - j) / np.maximum(fT - 1 - j, 1), 1.0)
            figures = (dcg / D[np.minimum(Pk, K)], H / Pk, H / K, np.where(fc > 0, 1.0 - miss, 0.0), rr)
            for f, v in enumerate(figures):
                out[f, q, seg] = v.mean()
    return out


def run(rows, domains, users, ks, reps, warmup, dev):
    rng = np.random.default_rng(0)
    score = rng.random(rows).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    rng.random(rows)                                                            # eval_ci_bench draws its second model here: the same set
    label = torch.from_numpy((rng.random(rows) < 0.1 + 0.3 * score).astype(np.int16)).to(dev)
    X = np.zeros((rows, 3), dtype=np.int32)
    X[:, 1] = rng.integers(0, domains, size=rows)
    X[:, 2] = (rng.zipf(1.3, size=rows) - 1) % users
    Xd = torch.from_numpy(X).to(dev)
    domain, user = Xd[:, 1], Xd[:, 2]

    calls = {"eval_gauc": lambda: eval_gauc(pred, label, user, users, domain, domains),
             "eval_rank": lambda: eval_rank(pred, label, user, users, domain, domains, ks)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    res = {"rows": rows, "domains": domains, "users": users, "ks": list(ks), "reps": reps}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    res["eval_rank_over_eval_gauc"] = res["eval_rank_ms_median"] / res["eval_gauc_ms_median"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = numpy_rank(pred, label, user, domain, domains, ks)
    res["numpy_rank_ms"] = (time.perf_counter() - t0) * 1e3
    r = calls["eval_rank"]()
    device = torch.stack(r[:len(RANK_FIGURES)]).cpu().numpy()
    both = ~np.isnan(host)
    assert np.array_equal(both, ~np.isnan(device))
    res["largest_device_minus_numpy"] = float(np.abs(device[both] - host[both]).max())
    res["users_counted"], res["users_left_out"] = int(r.counted[-1].item()), int(r.left_out[-1].item())
    for f, name in enumerate(RANK_FIGURES):
        res[name + "_all_rows"] = device[f, :, -1].tolist()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 5, 10, 50])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_bench needs a GPU")
    dev = torch.device("cuda:0")
    for domains in a.domains:
        print(json.dumps(run(a.rows, domains, a.users, tuple(a.ks), a.reps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
