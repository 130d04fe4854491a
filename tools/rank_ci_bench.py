"""Times eval_rank_ci — analytic, paired, and with 200 replicates unpaired and paired — beside eval_rank, eval_gauc_ci and eval_bootstrap
on the same evaluation set in the same run, and beside the same figures through the host in numpy: 500 000 rows, 50 000
Zipf-distributed users, 3 and 50 domains, ks = (1, 5, 10, 50) by default — the evaluation set of tools/rank_bench.py, with
tools/eval_ci_bench.py's second model as the paired vector.

The device calls alternate, 20 repetitions after a warm-up, each repetition between two device events (workspace allocation from the
caching allocator included, as a caller pays it); the numpy routes are timed once on the host clock after a device synchronisation,
the copies to the host included.  Reported beside the medians: the analytic call and ONE replicate (the difference between the call
with and without replicates, over their number) as multiples of eval_rank in that run.  Needs a GPU: there is no fallback.  Prints one
JSON line per domain count, with the largest difference between the device's and numpy's figures; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import (RANK_FIGURES, eval_bootstrap, eval_gauc_ci, eval_rank, eval_rank_ci, rank_discounts)  # noqa: E402

BOOT_T = (0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21, 0xffffffd4,
          0xfffffffc)                                                           # include/cdcmdr.h: floor(2^32 e^-1 sum_{j <= k} 1/j!)
MASK = (1 << 64) - 1


def _mix(x):
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def boot_weights(seed, r, users):
    """cdc_eval_bootstrap's weight of every user in replicate r (uint64 arithmetic wraps mod 2^64)"""
    base = _mix(np.array([(seed + 0x9E3779B97F4A7C15 * (r + 1)) & MASK], dtype=np.uint64))[0]
    u = (_mix(users.astype(np.uint64) + base) >> np.uint64(32)).astype(np.int64)
    return (u[:, None] >= np.asarray(BOOT_T, dtype=np.int64)[None, :]).sum(1)


def numpy_groups(s_all, y_all, u_all, d_all, n_domain, ks):
    """per segment (users counted [G], their values [G, 5, len(ks)]) through the host: tools/rank_bench.py's route — one lexsort per
    segment, the tie runs by reduceat, hit and mrr from the first run with a positive — kept per group"""
    D = rank_discounts(ks[-1]).numpy()
    out = []
    for seg in range(n_domain + 1):
        mk = slice(None) if seg == n_domain else d_all == seg
        y, u, s = y_all[mk], u_all[mk], s_all[mk]
        n = y.size
        if n == 0:
            out.append((np.zeros(0, np.int64), np.zeros((0, len(RANK_FIGURES), len(ks)))))
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
        vals = np.zeros((int(ok.sum()), len(RANK_FIGURES), len(ks)))
        if ok.any():
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
                for f, v in enumerate((dcg / D[np.minimum(Pk, K)], H / Pk, H / K, np.where(fc > 0, 1.0 - miss, 0.0), rr)):
                    vals[:, f, q] = v
        out.append((u[g_start][ok], vals))
    return out


def numpy_rank_ci(pred, pred_b, label, user, domain, n_domain, ks, n_rep, seed):
    """eval_rank_ci's outputs through the host (unweighted) -> (out [n_stat, 5, len(ks), seg], reps [n_vec, n_rep, 5, len(ks), seg] or None)"""
    y, u, d = label.cpu().numpy().astype(np.int64), user.cpu().numpy().astype(np.int64), domain.cpu().numpy()
    vecs = [numpy_groups(p.cpu().numpy() + np.float32(0), y, u, d, n_domain, ks) for p in ([pred] if pred_b is None else [pred, pred_b])]
    shape = (len(RANK_FIGURES), len(ks), n_domain + 1)
    out = np.full((6 if pred_b is not None else 2,) + shape, np.nan)
    reps = np.full((len(vecs), n_rep) + shape, np.nan) if n_rep else None
    for seg in range(n_domain + 1):
        users, G = vecs[0][seg][0], len(vecs[0][seg][0])
        if G == 0:
            continue
        scale = G / (G - 1) / G ** 2 if G > 1 else np.nan
        m = [v[seg][1] for v in vecs]
        for i, x in enumerate(m):
            out[2 * i, :, :, seg] = x.mean(0)
            out[2 * i + 1, :, :, seg] = scale * ((x - x.mean(0)) ** 2).sum(0)
        if pred_b is not None:
            x = m[0] - m[1]
            out[4, :, :, seg] = out[0, :, :, seg] - out[2, :, :, seg]
            out[5, :, :, seg] = scale * ((x - x.mean(0)) ** 2).sum(0)
        if n_rep:
            W = np.stack([boot_weights(seed, r, users) for r in range(n_rep)]).astype(np.float64)        # [n_rep, G]
            den = W.sum(1)
            for i, x in enumerate(m):
                with np.errstate(invalid="ignore", divide="ignore"):
                    reps[i, :, :, :, seg] = np.einsum("rg,gfk->rfk", W, x) / den[:, None, None]
    return out, reps


def run(rows, domains, users, ks, n_rep, reps, warmup, dev):
    rng = np.random.default_rng(0)
    score = rng.random(rows).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    pred_b = torch.from_numpy(np.clip(score + 0.05 * rng.standard_normal(rows).astype(np.float32), 0, 1)).to(dev)     # a second, close model
    label = torch.from_numpy((rng.random(rows) < 0.1 + 0.3 * score).astype(np.int16)).to(dev)
    X = np.zeros((rows, 3), dtype=np.int32)
    X[:, 1] = rng.integers(0, domains, size=rows)
    X[:, 2] = (rng.zipf(1.3, size=rows) - 1) % users
    Xd = torch.from_numpy(X).to(dev)
    domain, user = Xd[:, 1], Xd[:, 2]

    def ci(pb, r):
        return lambda: eval_rank_ci(pred, label, user, users, domain, domains, ks, pred_b=pb, n_rep=r, seed=1)
    calls = {"eval_rank": lambda: eval_rank(pred, label, user, users, domain, domains, ks),
             "eval_gauc_ci": lambda: eval_gauc_ci(pred, label, user, users, domain, domains),
             "eval_gauc_ci_paired": lambda: eval_gauc_ci(pred, label, user, users, domain, domains, pred_b=pred_b),
             "eval_bootstrap": lambda: eval_bootstrap(pred, label, user, users, domain, domains, n_rep, 1),
             "eval_bootstrap_paired": lambda: eval_bootstrap(pred, label, user, users, domain, domains, n_rep, 1, pred_b=pred_b),
             "eval_rank_ci": ci(None, 0), "eval_rank_ci_paired": ci(pred_b, 0),
             "eval_rank_ci_reps": ci(None, n_rep), "eval_rank_ci_paired_reps": ci(pred_b, n_rep)}

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
    res = {"rows": rows, "domains": domains, "users": users, "ks": list(ks), "n_rep": n_rep, "reps": reps}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    rank = res["eval_rank_ms_median"]
    res["analytic_over_eval_rank"] = res["eval_rank_ci_ms_median"] / rank
    res["paired_over_eval_rank"] = res["eval_rank_ci_paired_ms_median"] / rank
    res["one_replicate_over_eval_rank"] = (res["eval_rank_ci_reps_ms_median"] - res["eval_rank_ci_ms_median"]) / n_rep / rank
    res["one_paired_replicate_over_eval_rank"] = (res["eval_rank_ci_paired_reps_ms_median"] - res["eval_rank_ci_paired_ms_median"]) / n_rep / rank
    worst = 0.0
    for name, pb, r in (("numpy_analytic", None, 0), ("numpy_paired", pred_b, 0), ("numpy_reps", None, n_rep), ("numpy_paired_reps", pred_b, n_rep)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_out, host_reps = numpy_rank_ci(pred, pb, label, user, domain, domains, ks, r, 1)
        res[name + "_ms"] = (time.perf_counter() - t0) * 1e3
        got = ci(pb, r)()
        stats = [torch.stack(got[:5]), got.var] + ([got.fig_b, got.var_b, got.delta, got.var_delta] if pb is not None else [])
        pairs = [(torch.stack(stats).cpu().numpy(), host_out)]
        if r:
            pairs.append((torch.stack([got.reps] + ([got.reps_b] if pb is not None else [])).cpu().numpy(), host_reps))
        for device, host in pairs:
            both = ~np.isnan(host)
            assert np.array_equal(both, ~np.isnan(device)), name
            worst = max(worst, float(np.abs(device[both] - host[both]).max()))
    res["largest_device_minus_numpy"] = worst
    got = ci(pred_b, 0)()
    res["users_counted"] = int(got.counted[-1].item())
    for f, name in enumerate(RANK_FIGURES):
        res[name + "_all_rows"] = got[f][:, -1].cpu().tolist()
        res[name + "_all_rows_se"] = got.var[f, :, -1].sqrt().cpu().tolist()
        res[name + "_all_rows_delta"] = got.delta[f, :, -1].cpu().tolist()
        res[name + "_all_rows_delta_se"] = got.var_delta[f, :, -1].sqrt().cpu().tolist()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 5, 10, 50])
    ap.add_argument("--n-rep", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_ci_bench needs a GPU")
    dev = torch.device("cuda:0")
    for domains in a.domains:
        print(json.dumps(run(a.rows, domains, a.users, tuple(a.ks), a.n_rep, a.reps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
