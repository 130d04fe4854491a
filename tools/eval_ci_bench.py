"""Times eval_loss_ci and eval_gauc_ci, unpaired and paired, beside eval_metrics and eval_gauc on the same evaluation set and beside the
route through the host (the predictions copied back, the same figures in numpy): 500 000 rows with 3 and with 50 domains by default.

eval_metrics and eval_gauc are the yardsticks because they sort the same 2n keys.  eval_loss_ci sorts them once with a 4-byte payload
and walks every segment twice with one workgroup; paired it reads the second vector through the payload.  eval_gauc_ci runs
eval_gauc's sort, scans and sums and one more pass over the groups; paired it sorts and scans both vectors.  The device calls
alternate, 20 repetitions after a warm-up, each repetition between two device events (workspace allocation from the caching
allocator included, as a caller pays it); the numpy route is timed once per form with the copies to the host included.  Needs a
GPU: there is no fallback.  Prints one JSON line per domain count; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import eval_gauc, eval_gauc_ci, eval_loss_ci, eval_metrics  # noqa: E402


def numpy_loss_ci(pred, label, domain, n_domain, pred_b=None):
    """the figures of eval_loss_ci through the host: (loss, var[, delta, var_delta]) per domain and over all rows"""
    p, y, d = pred.cpu().numpy(), label.cpu().numpy() != 0, domain.cpu().numpy()
    q = None if pred_b is None else pred_b.cpu().numpy()
    eps = np.float32(np.finfo(np.float32).eps)

    def terms(v):
        return -np.log(np.clip(np.where(y, v, np.float32(1) - v), eps, np.float32(1) - eps).astype(np.float64))

    la, lb = terms(p), (None if q is None else terms(q))
    out = []
    for k in range(n_domain + 1):
        mk = slice(None) if k == n_domain else d == k
        for t in (la,) if lb is None else (la, la - lb):
            t = t[mk]
            m = t.size
            mean = t.mean() if m else np.nan
            out.append((mean, ((t - mean) ** 2).sum() / (m * (m - 1)) if m > 1 else np.nan))
    return out


def numpy_gauc_ci(pred, label, user, domain, n_domain, pred_b=None):
    """the figures of eval_gauc_ci through the host: one lexsort per vector and segment, rank sums by reduceat"""
    y, u, d = label.cpu().numpy().astype(np.int64), user.cpu().numpy().astype(np.int64), domain.cpu().numpy()
    vectors = [pred.cpu().numpy()] + ([] if pred_b is None else [pred_b.cpu().numpy()])
    out = []
    for k in range(n_domain + 1):
        mk = slice(None) if k == n_domain else d == k
        A = []
        for s in vectors:
            ys, us, ss = y[mk], u[mk], s[mk] + np.float32(0)
            n = ys.size
            if n == 0:
                A.append((np.zeros(0), np.zeros(0)))
                continue
            order = np.lexsort((ss, us))
            ys, us, ss = ys[order], us[order], ss[order]
            new_g = np.r_[True, us[1:] != us[:-1]]
            new_t = new_g | np.r_[True, ss[1:] != ss[:-1]]
            g_start, t_start = np.flatnonzero(new_g), np.flatnonzero(new_t)
            t_end = np.r_[t_start[1:], n] - 1
            run_of, grp_of = np.cumsum(new_t) - 1, np.cumsum(new_g) - 1
            h = g_start[grp_of]
            twice = (t_start[run_of] - h) + (t_end[run_of] - h) + 2
            S2 = np.add.reduceat(np.where(ys == 1, twice, 0), g_start)
            P = np.add.reduceat(ys, g_start)
            rows = np.diff(np.r_[g_start, n])
            N = rows - P
            ok = (P > 0) & (N > 0)
            A.append(((S2 - P * (P + 1))[ok] / (2.0 * P[ok] * N[ok]), rows[ok].astype(np.float64)))
        for v, w in [A[0]] + ([(A[0][0] - A[1][0], A[0][1])] if len(A) > 1 else []):
            K = v.size
            G = (w * v).sum() / w.sum() if K else np.nan
            out.append((G, K / (K - 1) * ((w * (v - G)) ** 2).sum() / w.sum() ** 2 if K > 1 else np.nan))
    return out


def run(rows, domains, users, reps, warmup, dev):
    rng = np.random.default_rng(0)
    score = rng.random(rows).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    close = np.clip(score + (rng.random(rows).astype(np.float32) - np.float32(0.5)) * np.float32(1e-3), 0, 1).astype(np.float32)
    pred_b = torch.from_numpy(close).to(dev)                                    # a close second model
    label = torch.from_numpy((rng.random(rows) < 0.1 + 0.3 * score).astype(np.int16)).to(dev)
    X = np.zeros((rows, 3), dtype=np.int32)
    X[:, 1] = rng.integers(0, domains, size=rows)
    X[:, 2] = (rng.zipf(1.3, size=rows) - 1) % users
    Xd = torch.from_numpy(X).to(dev)
    domain, user = Xd[:, 1], Xd[:, 2]

    calls = {"eval_metrics": lambda: eval_metrics(pred, label, domain, domains),
             "eval_loss_ci": lambda: eval_loss_ci(pred, label, domain, domains),
             "eval_loss_ci_paired": lambda: eval_loss_ci(pred, label, domain, domains, pred_b=pred_b),
             "eval_gauc": lambda: eval_gauc(pred, label, user, users, domain, domains),
             "eval_gauc_ci": lambda: eval_gauc_ci(pred, label, user, users, domain, domains),
             "eval_gauc_ci_paired": lambda: eval_gauc_ci(pred, label, user, users, domain, domains, pred_b=pred_b)}
    host = {"numpy_loss_ci": lambda: numpy_loss_ci(pred, label, domain, domains),
            "numpy_loss_ci_paired": lambda: numpy_loss_ci(pred, label, domain, domains, pred_b),
            "numpy_gauc_ci": lambda: numpy_gauc_ci(pred, label, user, domain, domains),
            "numpy_gauc_ci_paired": lambda: numpy_gauc_ci(pred, label, user, domain, domains, pred_b)}

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
    res = {"rows": rows, "domains": domains, "users": users, "reps": reps}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    for k, fn in host.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        figures = fn()
        res[k + "_ms"] = (time.perf_counter() - t0) * 1e3
        res[k + "_all_rows"] = [float(x) for x in figures[-1]]
    lci, gci = calls["eval_loss_ci_paired"](), calls["eval_gauc_ci_paired"]()
    res.update({"loss": lci.loss[-1].item(), "loss_se": lci.var[-1].sqrt().item(), "loss_delta": lci.delta[-1].item(),
                "loss_delta_se": lci.var_delta[-1].sqrt().item(), "gauc": gci.gauc[-1].item(), "gauc_se": gci.var[-1].sqrt().item(),
                "gauc_delta": gci.delta[-1].item(), "gauc_delta_se": gci.var_delta[-1].sqrt().item(),
                "users_counted": int(gci.counted[-1].item())})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_ci_bench needs a GPU")
    dev = torch.device("cuda:0")
    for domains in a.domains:
        print(json.dumps(run(a.rows, domains, a.users, a.reps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
