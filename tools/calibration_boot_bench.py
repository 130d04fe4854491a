"""Times eval_calibration_bootstrap (clustered by user, 200 replicates, 10 bins by default), single and paired, beside
eval_bootstrap at the same shape, beside eval_calibration (one replicate's cost if the bootstrap were a loop over it) and beside the
route through the host: the predictions copied back and the four figures recomputed per replicate in numpy from the weight recipe.
500 000 rows of 50 000 Zipf-distributed users with 3 and with 50 domains by default.

The device calls alternate, 20 repetitions after a warm-up of every shape, each repetition between two device events (workspace
allocation from the caching allocator included, as a caller pays it).  The numpy route sorts every segment once, as the device does,
and reweights per replicate (np.repeat of the sorted rows for the equal-mass bins); it is timed ONCE per form, at --host-reps
replicates (5 by default, not 200), copies to the host included, and reported per replicate.  `host_device_max_rel_diff` holds the
device's replicates to the host route's.  Needs a GPU: there is no fallback.  Prints one JSON line per domain count; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from bootstrap_exact import weights  # noqa: E402  (tests/bootstrap_exact.py: the weight recipe of include/cdcmdr.h in numpy)
from cdcmdr_amd.evaluate import eval_bootstrap, eval_calibration, eval_calibration_bootstrap, summarize_bootstrap  # noqa: E402

ONE = float(1 << 32)


def numpy_calibration_bootstrap(pred, label, user, n_user, domain, n_domain, n_bins, n_rep, seed, pred_b=None):
    """eval_calibration_bootstrap's replicates through the host -> {figure: [n_rep, n_domain + 1]} in float64 arithmetic (sums of
    q = rint(p 2^32) below 2^53 here: exact)"""
    y, u, d = label.cpu().numpy().astype(np.int64), user.cpu().numpy().astype(np.int64), domain.cpu().numpy()
    vectors = [pred.cpu().numpy()] + ([] if pred_b is None else [pred_b.cpu().numpy()])
    K = n_bins
    seg_rows = [np.arange(y.size) if k == n_domain else np.flatnonzero(d == k) for k in range(n_domain + 1)]
    prepared = []
    for s in vectors:
        per_seg = []
        for rows in seg_rows:
            order = rows[np.lexsort((y[rows], s[rows]))]
            q = np.rint(s[order].astype(np.float64) * ONE)
            bw = np.minimum(np.floor(s[order].astype(np.float64) * K).astype(np.int64), K - 1)
            per_seg.append((order, q, bw, y[order].astype(np.float64)))
        prepared.append(per_seg)
    names = ["pcoc", "brier", "ece", "ece_q"] + (["pcoc_b", "brier_b", "ece_b", "ece_q_b"] if pred_b is not None else [])
    out = {k: np.full((n_rep, n_domain + 1), np.nan) for k in names}
    for r in range(n_rep):
        w = weights(seed, r, np.arange(n_user))[u]
        for v, per_seg in enumerate(prepared):
            sfx = "_b" if v else ""
            for k, (order, q, bw, yo) in enumerate(per_seg):
                wo = w[order]
                W = int(wo.sum())
                if W == 0:
                    continue
                Wp = float((wo * yo).sum())
                if Wp > 0:
                    out["pcoc" + sfx][r, k] = (wo * q).sum() / (Wp * ONE)
                out["brier" + sfx][r, k] = (wo * ((q - yo * ONE) / ONE) ** 2).sum() / W
                gap = np.abs(np.bincount(bw, wo * q, K) - np.bincount(bw, wo * yo, K) * ONE).sum()
                out["ece" + sfx][r, k] = gap / (W * ONE)
                bq = ((np.arange(1, W + 1) * K - 1) // W)                    # the mass bin of every expanded position
                qe, ye = np.repeat(q, wo), np.repeat(yo, wo)
                gap = np.abs(np.bincount(bq, qe, K) - np.bincount(bq, ye, K) * ONE).sum()
                out["ece_q" + sfx][r, k] = gap / (W * ONE)
    return out


def run(rows, domains, users, n_rep, n_bins, host_reps, reps, warmup, dev):
    rng = np.random.default_rng(0)
    X = np.zeros((rows, 3), dtype=np.int32)
    X[:, 1] = rng.integers(0, domains, size=rows)
    X[:, 2] = (rng.zipf(1.3, size=rows) - 1) % users
    effect = rng.normal(size=users).astype(np.float32)[X[:, 2]]             # a user effect in the score: rows of a user correlate
    score = (1 / (1 + np.exp(-(rng.normal(size=rows).astype(np.float32) + effect)))).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    shifted = (1 / (1 + np.exp(-(np.log(score / (1 - score)) - np.float32(0.3))))).astype(np.float32)
    pred_b = torch.from_numpy(np.clip(shifted, 0, 1)).to(dev)               # the same model under a bias shift
    label = torch.from_numpy((rng.random(rows) < 0.05 + 0.5 * score).astype(np.int16)).to(dev)
    Xd = torch.from_numpy(X).to(dev)
    domain, user = Xd[:, 1], Xd[:, 2]

    calls = {"eval_calibration": lambda: eval_calibration(pred, label, domain, domains, n_bins),
             "eval_bootstrap": lambda: eval_bootstrap(pred, label, user, users, domain, domains, n_rep, 0),
             "eval_calibration_bootstrap": lambda: eval_calibration_bootstrap(pred, label, user, users, domain, domains, n_bins, n_rep, 0),
             "eval_calibration_bootstrap_paired": lambda: eval_calibration_bootstrap(pred, label, user, users, domain, domains, n_bins,
                                                                                     n_rep, 0, pred_b=pred_b),
             "eval_calibration_bootstrap_rows": lambda: eval_calibration_bootstrap(pred, label, None, None, domain, domains, n_bins,
                                                                                   n_rep, 0)}

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
    res = {"rows": rows, "domains": domains, "users": users, "n_rep": n_rep, "n_bins": n_bins, "reps": reps}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    for k in ("eval_calibration_bootstrap", "eval_calibration_bootstrap_paired", "eval_calibration_bootstrap_rows"):
        res[k + "_ms_per_replicate"] = res[k + "_ms_median"] / n_rep
    res["replicate_over_eval_calibration"] = res["eval_calibration_bootstrap_ms_per_replicate"] / res["eval_calibration_ms_median"]
    res["over_eval_bootstrap"] = res["eval_calibration_bootstrap_ms_median"] / res["eval_bootstrap_ms_median"]
    for k, pb in (("numpy_calibration_bootstrap", None), ("numpy_calibration_bootstrap_paired", pred_b)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = numpy_calibration_bootstrap(pred, label, user, users, domain, domains, n_bins, host_reps, 0, pb)
        res[k + "_ms"] = (time.perf_counter() - t0) * 1e3
        res[k + "_replicates"] = host_reps
        res[k + "_ms_per_replicate"] = res[k + "_ms"] / host_reps
    boot = calls["eval_calibration_bootstrap_paired"]()
    res["host_device_max_rel_diff"] = {k: float(np.nanmax(np.abs(host[k] / getattr(boot, k)[:host_reps].cpu().numpy() - 1))) for k in host}
    cal = calls["eval_calibration"]()
    for k, point in (("brier", cal.brier), ("ece", cal.ece), ("ece_q", cal.ece_q), ("pcoc", cal.pcoc)):
        se, lo, hi, _ = summarize_bootstrap(getattr(boot, k))
        res[k] = point[-1].item()
        res[k + "_boot_se"], res[k + "_boot_lo"], res[k + "_boot_hi"] = se[-1].item(), lo[-1].item(), hi[-1].item()
    res["ece_delta_boot_se"] = summarize_bootstrap(boot.ece - boot.ece_b)[0][-1].item()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--n-rep", type=int, default=200)
    ap.add_argument("--n-bins", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calibration_boot_bench needs a GPU")
    dev = torch.device("cuda:0")
    for domains in a.domains:
        print(json.dumps(run(a.rows, domains, a.users, a.n_rep, a.n_bins, a.host_reps, a.reps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
