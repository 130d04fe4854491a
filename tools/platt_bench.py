"""Times eval_platt_fit (the three methods) and eval_platt_apply beside eval_isotonic_fit and eval_calibration on the same synthetic
CTR-like rows: 500 000 rows (the README's evaluation-set size) with 3 and with 50 domains by default.

eval_isotonic_fit and eval_calibration are the yardsticks: they key every row twice and sort the same 2n keys over the same bits;
the Platt fit adds to that sort one launch that writes z, max_iter + 1 pass launches (a converged segment's workgroups return at
once) and one final launch.  The calls alternate, 20 repetitions after a warm-up, each repetition between two device events
(workspace allocation from the caching allocator included, as a caller pays it).  `passes` is the largest number of Newton steps a
segment took; the fit is timed a second time with max_iter set to exactly that, so the difference to the default of 32 is what the
launches that find every segment converged cost.  Where sklearn imports, the host round trip the device path replaces is timed too
(once): scores, labels and domains to the host, a LogisticRegression per domain and one over all rows, the recalibrated predictions
back to the device.  Needs a GPU: there is no fallback.  Prints one JSON line per domain count; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd import _lib  # noqa: E402
from cdcmdr_amd.evaluate import PLATT_METHODS, eval_calibration, eval_isotonic_fit, eval_platt_apply, eval_platt_fit  # noqa: E402


def host_round_trip(pred, label, domain, n_domain):
    from sklearn.linear_model import LogisticRegression
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, y, d = pred.cpu().numpy().astype(np.float64), label.cpu().numpy(), domain.cpu().numpy()
    z = np.clip(np.log(p) - np.log1p(-p), -16.0, 16.0)[:, None]
    out = np.empty(len(p), np.float32)
    LogisticRegression(penalty=None).fit(z, y)                             # the map of all rows: the fallback
    order = np.argsort(d, kind="stable")                                   # groupby
    bounds = np.searchsorted(d[order], np.arange(n_domain + 1))
    for s in range(n_domain):
        idx = order[bounds[s]:bounds[s + 1]]
        if len(idx) and 0 < y[idx].sum() < len(idx):
            out[idx] = LogisticRegression(penalty=None).fit(z[idx], y[idx]).predict_proba(z[idx])[:, 1]
    torch.from_numpy(out).to(pred.device)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench(rows, n_domain, reps, warmup, host_reps, dev):
    rng = np.random.default_rng(0)
    score = (rng.random(rows) ** 5).astype(np.float32)                     # skewed like CTR predictions: most mass below 0.1
    score[rng.random(rows) < 0.1] = np.float32(0.03125)                    # a tie run
    pred = torch.from_numpy(score).to(dev)
    label = torch.from_numpy((rng.random(rows) < 0.03 + 0.6 * score).astype(np.int16)).to(dev)
    X = np.zeros((rows, 2), dtype=np.int32)
    X[:, 1] = rng.integers(0, n_domain, size=rows)
    domain = torch.from_numpy(X).to(dev)[:, 1]
    fits = {m: eval_platt_fit(pred, label, domain, n_domain, method=m) for m in PLATT_METHODS}
    passes = {m: int(f.iterations.max().item()) for m, f in fits.items()}
    converged = {m: bool((f.status & 3 != 0).all().item()) for m, f in fits.items()}       # CONVERGED or EMPTY everywhere

    calls = {}
    for m in PLATT_METHODS:
        calls[f"eval_platt_fit[{m}]"] = lambda m=m: eval_platt_fit(pred, label, domain, n_domain, method=m)
        calls[f"eval_platt_fit[{m}, max_iter=passes]"] = lambda m=m: eval_platt_fit(pred, label, domain, n_domain, method=m, max_iter=max(1, passes[m]))
    calls["eval_platt_apply"] = lambda: eval_platt_apply(pred, fits["platt"], domain, n_domain)
    calls["eval_isotonic_fit"] = lambda: eval_isotonic_fit(pred, label, domain, n_domain)
    calls["eval_calibration"] = lambda: eval_calibration(pred, label, domain, n_domain, 10)

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
    lib = _lib.load()
    res = {"rows": rows, "domains": n_domain, "reps": reps, "passes": passes, "all_converged": converged}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    res.update({"platt_over_isotonic": res["eval_platt_fit[platt]_ms_median"] / res["eval_isotonic_fit_ms_median"],
                "err": int(eval_platt_fit.last_err.item()),
                "workspace_mib": {"eval_platt_fit": lib.cdc_eval_platt_fit_workspace_bytes(rows, n_domain) / 2 ** 20,
                                  "eval_isotonic_fit": lib.cdc_eval_isotonic_fit_workspace_bytes(rows, n_domain) / 2 ** 20,
                                  "eval_calibration": lib.cdc_eval_calibration_workspace_bytes(rows, n_domain, 10) / 2 ** 20}})
    res["host_sklearn_ms_median"] = None                                    # not asked for (--host-reps 0), or no sklearn here
    if host_reps > 0:
        try:
            import sklearn.linear_model  # noqa: F401
        except ImportError:
            return res
        res["host_sklearn_ms_median"] = statistics.median(host_round_trip(pred, label, domain, n_domain) for _ in range(host_reps))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("platt_bench needs a GPU")
    for n_domain in a.domains:
        print(json.dumps(bench(a.rows, n_domain, a.reps, a.warmup, a.host_reps, torch.device("cuda:0"))), flush=True)


if __name__ == "__main__":
    main()
