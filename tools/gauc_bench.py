"""Times eval_gauc beside eval_metrics on the same evaluation set: 4 M rows, 1 M users, 3 domains by default.

eval_metrics is the yardstick because it sorts the same 2n keys (every row keyed once per domain segment and once for the whole
set); the difference is what follows the sort.  The two calls alternate, 20 repetitions after a warm-up, each repetition between
two device events (workspace allocation from the caching allocator included, as a caller pays it).  Needs a GPU: there is no
fallback.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import eval_gauc, eval_metrics  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--domains", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weighted", action="store_true", help="pass a user_weight array instead of the row-count default")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gauc_bench needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.random(a.rows).astype(np.float32)).to(dev)
    label = torch.from_numpy((rng.random(a.rows) < 0.25).astype(np.int16)).to(dev)
    X = np.zeros((a.rows, 2), dtype=np.int32)
    X[:, 0] = np.minimum(rng.zipf(1.3, size=a.rows) - 1, a.users - 1)         # a few heavy users, a long tail of one-row users
    X[:, 1] = rng.integers(0, a.domains, size=a.rows)
    Xd = torch.from_numpy(X).to(dev)
    user, domain = Xd[:, 0], Xd[:, 1]
    w = torch.from_numpy(0.5 + rng.random(a.users)).to(dev) if a.weighted else None

    def gauc():
        return eval_gauc(pred, label, user, a.users, domain, a.domains, w)

    def metrics():
        return eval_metrics(pred, label, domain, a.domains)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        gauc()
        metrics()
    torch.cuda.synchronize()
    t_g, t_m = [], []
    for _ in range(a.reps):
        t_g.append(timed(gauc))
        t_m.append(timed(metrics))
    g, counted, left = gauc()
    res = {"rows": a.rows, "users": a.users, "domains": a.domains, "reps": a.reps, "weighted": a.weighted,
           "eval_gauc_ms_median": statistics.median(t_g), "eval_gauc_ms_min": min(t_g), "eval_gauc_ms_max": max(t_g),
           "eval_metrics_ms_median": statistics.median(t_m), "eval_metrics_ms_min": min(t_m), "eval_metrics_ms_max": max(t_m),
           "ratio_median": statistics.median(t_g) / statistics.median(t_m),
           "gauc": g.cpu().tolist(), "users_counted": counted.cpu().tolist(), "users_left_out": left.cpu().tolist(),
           "workspace_mib": {"eval_gauc": eval_gauc_ws(a) / 2 ** 20, "eval_metrics": eval_metrics_ws(a) / 2 ** 20}}
    print(json.dumps(res))


def eval_gauc_ws(a):
    from cdcmdr_amd import _lib
    return _lib.load().cdc_eval_gauc_workspace_bytes(a.rows, a.domains, a.users)


def eval_metrics_ws(a):
    from cdcmdr_amd import _lib
    return _lib.load().cdc_eval_workspace_bytes(a.rows, a.domains)


if __name__ == "__main__":
    main()
