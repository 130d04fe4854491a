"""Times eval_auc_ci, unpaired and paired, beside eval_metrics on the same evaluation set: 4 M rows, 3 domains by default.

eval_metrics is the yardstick because it sorts the same 2n keys (every row keyed once per domain segment and once for the whole
set); the unpaired call sorts them once with a 4-byte payload and adds a scan, the paired call does so for both score vectors.
The three calls alternate, 20 repetitions after a warm-up, each repetition between two device events (workspace allocation from the
caching allocator included, as a caller pays it).  Needs a GPU: there is no fallback.  Prints one JSON line; no threshold."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd import _lib  # noqa: E402
from cdcmdr_amd.evaluate import eval_auc_ci, eval_metrics  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--domains", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("delong_bench needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    score = rng.random(a.rows).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    pred_b = torch.from_numpy((score + (rng.random(a.rows).astype(np.float32) - 0.5) * 1e-3).astype(np.float32)).to(dev)   # a close second model
    label = torch.from_numpy((rng.random(a.rows) < 0.1 + 0.3 * score).astype(np.int16)).to(dev)
    X = np.zeros((a.rows, 2), dtype=np.int32)
    X[:, 1] = rng.integers(0, a.domains, size=a.rows)
    domain = torch.from_numpy(X).to(dev)[:, 1]

    calls = {"eval_auc_ci": lambda: eval_auc_ci(pred, label, domain, a.domains),
             "eval_auc_ci_paired": lambda: eval_auc_ci(pred, label, domain, a.domains, pred_b=pred_b),
             "eval_metrics": lambda: eval_metrics(pred, label, domain, a.domains)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    ci = calls["eval_auc_ci_paired"]()
    lib = _lib.load()
    res = {"rows": a.rows, "domains": a.domains, "reps": a.reps}
    for k, v in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(v), min(v), max(v)
    base = res["eval_metrics_ms_median"]
    res.update({"ratio_unpaired": res["eval_auc_ci_ms_median"] / base, "ratio_paired": res["eval_auc_ci_paired_ms_median"] / base,
                "auc": ci.auc.cpu().tolist(), "se": ci.var.sqrt().cpu().tolist(), "delta": ci.delta.cpu().tolist(),
                "delta_se": ci.var_delta.sqrt().cpu().tolist(),
                "workspace_mib": {"eval_auc_ci": lib.cdc_eval_auc_delong_workspace_bytes(a.rows, a.domains, 0) / 2 ** 20,
                                  "eval_auc_ci_paired": lib.cdc_eval_auc_delong_workspace_bytes(a.rows, a.domains, 1) / 2 ** 20,
                                  "eval_metrics": lib.cdc_eval_workspace_bytes(a.rows, a.domains) / 2 ** 20}})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
