"""Times eval_bootstrap (clustered by user, 200 replicates by default), single and paired, beside eval_metrics, eval_auc_ci,
eval_loss_ci and eval_gauc_ci on the same evaluation set and beside the route through the host (the predictions copied back, the
same replicates in numpy): 500 000 rows of 50 000 Zipf-distributed users with 3 and with 50 domains by default.

eval_metrics is the yardstick: it sorts the same 2n keys once, which is what one replicate would cost if the bootstrap were a loop
over it; `replicate_over_eval_metrics` is (eval_bootstrap's time / n_rep) / eval_metrics' time.  `eval_bootstrap_rows` is the same
call without a cluster column (row bootstrap, no GAUC).  The device calls alternate, 20 repetitions after a warm-up, each repetition
between two device events (workspace allocation from the caching allocator included, as a caller pays it).  The numpy route sorts
every segment once, as the device does, and reweights per replicate; it is timed ONCE per form, at --host-reps replicates (20 by
default, not 200), copies to the host included, and reported per replicate as well.  Needs a GPU: there is no fallback.  Prints one
JSON line per domain count; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import (eval_auc_ci, eval_bootstrap, eval_gauc_ci, eval_loss_ci, eval_metrics,  # noqa: E402
                                 summarize_bootstrap)

T = np.array([0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21,
              0xffffffd4, 0xfffffffc], dtype=np.int64)
MASK = (1 << 64) - 1


def _mix(x):
    x &= MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def weights(seed, r, clusters):
    """include/cdcmdr.h's weight recipe on an array of cluster ids (uint64 arithmetic wraps mod 2^64)"""
    x = clusters.astype(np.uint64) + np.uint64(_mix(seed + 0x9E3779B97F4A7C15 * (r + 1)))
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return np.searchsorted(T, (x >> np.uint64(32)).astype(np.int64), side="right")


def numpy_bootstrap(pred, label, user, n_user, domain, n_domain, n_rep, seed, pred_b=None):
    """eval_bootstrap's replicates through the host -> {stat: [n_rep, n_domain + 1]}.  Per vector and segment the rows are sorted and
    the users' AUCs formed once; a replicate draws one weight per user and reweights."""
    y, u, d = label.cpu().numpy().astype(np.int64), user.cpu().numpy().astype(np.int64), domain.cpu().numpy()
    vectors = [pred.cpu().numpy()] + ([] if pred_b is None else [pred_b.cpu().numpy()])
    eps = np.float32(np.finfo(np.float32).eps)
    seg_rows = [np.arange(y.size) if k == n_domain else np.flatnonzero(d == k) for k in range(n_domain + 1)]
    prepared = []
    for s in vectors:
        terms = -np.log(np.clip(np.where(y != 0, s, np.float32(1) - s), eps, np.float32(1) - eps).astype(np.float64))
        per_seg = []
        for rows in seg_rows:
            ss = s[rows] + np.float32(0)
            order = rows[np.argsort(ss, kind="stable")]
            run = np.cumsum(np.r_[True, s[order][1:] != s[order][:-1]]) - 1 if order.size else np.zeros(0, dtype=np.int64)
            ys, us = y[rows], u[rows]
            o2 = np.lexsort((ss, us))                                      # the users' unweighted AUCs, once
            ys2, us2, ss2 = ys[o2], us[o2], ss[o2]
            gauc = (np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0))
            if rows.size:
                new_g = np.r_[True, us2[1:] != us2[:-1]]
                new_t = new_g | np.r_[True, ss2[1:] != ss2[:-1]]
                g_start, t_start = np.flatnonzero(new_g), np.flatnonzero(new_t)
                t_end = np.r_[t_start[1:], rows.size] - 1
                run_of, grp_of = np.cumsum(new_t) - 1, np.cumsum(new_g) - 1
                h = g_start[grp_of]
                twice = (t_start[run_of] - h) + (t_end[run_of] - h) + 2
                S2, P = np.add.reduceat(np.where(ys2 == 1, twice, 0), g_start), np.add.reduceat(ys2, g_start)
                cnt = np.diff(np.r_[g_start, rows.size])
                ok = (P > 0) & (cnt - P > 0)
                gauc = (us2[g_start][ok], (S2 - P * (P + 1))[ok] / (2.0 * P[ok] * (cnt - P)[ok]), cnt[ok].astype(np.float64))
            per_seg.append((order, run, gauc))
        prepared.append((terms, per_seg))
    names = ["auc", "loss", "gauc"] + (["auc_b", "loss_b", "gauc_b"] if pred_b is not None else [])
    out = {k: np.full((n_rep, n_domain + 1), np.nan) for k in names}
    for r in range(n_rep):
        wu = weights(seed, r, np.arange(n_user))
        w = wu[u]
        for v, (terms, per_seg) in enumerate(prepared):
            sfx = "_b" if v else ""
            for k, (order, run, (gu, ga, gw)) in enumerate(per_seg):
                wo, yo = w[order], y[order]
                W, Wp = wo.sum(), (wo * yo).sum()
                if Wp > 0 and W - Wp > 0:
                    wp_run = np.bincount(run, wo * yo)
                    wn_run = np.bincount(run, wo * (1 - yo))
                    below = np.cumsum(wn_run) - wn_run
                    out["auc" + sfx][r, k] = (wp_run * (2 * below + wn_run)).sum() / (2.0 * Wp * (W - Wp))
                    out["loss" + sfx][r, k] = (wo * terms[order]).sum() / W
                ww = wu[gu] * gw
                if ww.sum() > 0:
                    out["gauc" + sfx][r, k] = (ww * ga).sum() / ww.sum()
    return out


def run(rows, domains, users, n_rep, host_reps, reps, warmup, dev):
    rng = np.random.default_rng(0)
    X = np.zeros((rows, 3), dtype=np.int32)
    X[:, 1] = rng.integers(0, domains, size=rows)
    X[:, 2] = (rng.zipf(1.3, size=rows) - 1) % users
    effect = rng.normal(size=users).astype(np.float32)[X[:, 2]]             # a user effect in the score: rows of a user correlate
    score = (1 / (1 + np.exp(-(rng.normal(size=rows).astype(np.float32) + effect)))).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    close = np.clip(score + (rng.random(rows).astype(np.float32) - np.float32(0.5)) * np.float32(1e-3), 0, 1).astype(np.float32)
    pred_b = torch.from_numpy(close).to(dev)                                    # a close second model
    label = torch.from_numpy((rng.random(rows) < 0.05 + 0.5 * score).astype(np.int16)).to(dev)
    Xd = torch.from_numpy(X).to(dev)
    domain, user = Xd[:, 1], Xd[:, 2]

    calls = {"eval_metrics": lambda: eval_metrics(pred, label, domain, domains),
             "eval_auc_ci": lambda: eval_auc_ci(pred, label, domain, domains),
             "eval_loss_ci": lambda: eval_loss_ci(pred, label, domain, domains),
             "eval_gauc_ci": lambda: eval_gauc_ci(pred, label, user, users, domain, domains),
             "eval_bootstrap": lambda: eval_bootstrap(pred, label, user, users, domain, domains, n_rep, 0),
             "eval_bootstrap_paired": lambda: eval_bootstrap(pred, label, user, users, domain, domains, n_rep, 0, pred_b=pred_b),
             "eval_bootstrap_rows": lambda: eval_bootstrap(pred, label, None, None, domain, domains, n_rep, 0)}

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
    res = {"rows": rows, "domains": domains, "users": users, "n_rep": n_rep, "reps": reps}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    for k in ("eval_bootstrap", "eval_bootstrap_paired", "eval_bootstrap_rows"):
        res[k + "_ms_per_replicate"] = res[k + "_ms_median"] / n_rep
    res["replicate_over_eval_metrics"] = res["eval_bootstrap_ms_per_replicate"] / res["eval_metrics_ms_median"]
    res["rows_replicate_over_eval_metrics"] = res["eval_bootstrap_rows_ms_per_replicate"] / res["eval_metrics_ms_median"]
    for k, pb in (("numpy_bootstrap", None), ("numpy_bootstrap_paired", pred_b)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = numpy_bootstrap(pred, label, user, users, domain, domains, host_reps, 0, pb)
        res[k + "_ms"] = (time.perf_counter() - t0) * 1e3
        res[k + "_replicates"] = host_reps
        res[k + "_ms_per_replicate"] = res[k + "_ms"] / host_reps
    boot = calls["eval_bootstrap_paired"]()
    ci, lci, gci = calls["eval_auc_ci"](), calls["eval_loss_ci"](), calls["eval_gauc_ci"]()
    res["host_device_max_abs_diff"] = {k: float(np.nanmax(np.abs(host[k] - getattr(boot, k)[:host_reps].cpu().numpy()))) for k in host}
    se = {k: summarize_bootstrap(getattr(boot, k))[0][-1].item() for k in ("auc", "loss", "gauc")}
    res.update({"auc_boot_se": se["auc"], "auc_delong_se": ci.var[-1].sqrt().item(), "loss_boot_se": se["loss"],
                "loss_se": lci.var[-1].sqrt().item(), "gauc_boot_se": se["gauc"], "gauc_se": gci.var[-1].sqrt().item(),
                "auc_delta_boot_se": summarize_bootstrap(boot.auc - boot.auc_b)[0][-1].item()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--n-rep", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bootstrap_bench needs a GPU")
    dev = torch.device("cuda:0")
    for domains in a.domains:
        print(json.dumps(run(a.rows, domains, a.users, a.n_rep, a.host_reps, a.reps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
