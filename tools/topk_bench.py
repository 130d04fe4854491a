"""Times eval_topk — every user's k best rows, per (domain, user) — beside eval_rank on the same rows, beside a torch-ops device route
that produces the same lists from stable torch.sort calls, and beside the route through the host (numpy lexsort), all in one run:
500 000 rows, 50 000 Zipf-distributed users, 3 and 50 domains, k = 10, with and without de-duplication over 20 000 item ids — the
evaluation set of tools/rank_bench.py with an item column.

The yardsticks are eval_rank (GAUC's sort of 2n keys, one scan and the group walk: the call whose ranking eval_topk hands back) and
the torch-ops route (what a caller writes without the library and without leaving the device: two stable sorts without items, five
with).  The three device routes alternate, 20 repetitions after a warm-up, each repetition between two device events with the
result's counts read back inside it (workspace and output allocation from the caching allocator included, as a caller pays them);
the numpy route is timed once, the copies to the host included.  The three results are compared field by field; the run aborts when
they differ.  Needs a GPU: there is no fallback.  Prints one JSON line per (domain count, item column); no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import eval_rank, eval_topk  # noqa: E402


def _cut_torch(order, g, k, users):
    """rows in (group, rank) order and their group ids -> the six fields of a TopK"""
    n = order.numel()
    pos = torch.arange(n, device=order.device)
    head = torch.ones(n, dtype=torch.bool, device=order.device)
    head[1:] = g[1:] != g[:-1]
    first = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0).values
    keep = pos - first < k
    heads = pos[head]
    kept_before = torch.cumsum(keep, 0) - keep.to(torch.int64)
    start = torch.cat([kept_before[heads], keep.sum().reshape(1)])
    rows = torch.diff(torch.cat([heads, torch.tensor([n], device=order.device)]))
    gid = g[heads]
    return gid // users, gid % users, start, rows, order[keep]


def torch_topk(pred, user, domain, item, users, k):
    s = pred + 0.0                                                          # -0.0 -> +0.0: one score
    g = domain.to(torch.int64) * users + user.to(torch.int64)
    by_score = torch.sort(s, descending=True, stable=True).indices           # (score desc, row)
    if item is not None:
        it = item.to(torch.int64)
        o = by_score[torch.sort(it[by_score], stable=True).indices]          # (item, score desc, row)
        o = o[torch.sort(g[o], stable=True).indices]                         # (group, item, score desc, row)
        go, io = g[o], it[o]
        best = torch.ones(o.numel(), dtype=torch.bool, device=o.device)
        best[1:] = (go[1:] != go[:-1]) | (io[1:] != io[:-1])
        w = o[best]                                                          # one row per (group, item), in (group, item) order
        by_score = w[torch.sort(s[w], descending=True, stable=True).indices]  # (score desc, group, item)
    order = by_score[torch.sort(g[by_score], stable=True).indices]           # (group, score desc, [item,] row)
    d, u, start, rows, row = _cut_torch(order, g[order], k, users)
    return d, u, start, rows, row, pred[row]


def numpy_topk(pred, user, domain, item, users, k):
    s0 = pred.cpu().numpy()
    s = s0 + np.float32(0)
    g = domain.cpu().numpy().astype(np.int64) * users + user.cpu().numpy().astype(np.int64)
    if item is None:
        order = np.lexsort((-s, g))                                         # lexsort is stable: ties in row order
    else:
        it = item.cpu().numpy().astype(np.int64)
        o = np.lexsort((-s, it, g))
        best = np.r_[True, (g[o][1:] != g[o][:-1]) | (it[o][1:] != it[o][:-1])]
        w = o[best]
        order = w[np.lexsort((it[w], -s[w], g[w]))]
    go = g[order]
    n = order.size
    head = np.r_[True, go[1:] != go[:-1]]
    heads = np.flatnonzero(head)
    rank = np.arange(n) - np.maximum.accumulate(np.where(head, np.arange(n), 0))
    keep = rank < k
    start = np.r_[(np.cumsum(keep) - keep)[heads], keep.sum()]
    row = order[keep]
    return go[heads] // users, go[heads] % users, start, np.diff(np.r_[heads, n]), row, s0[row]


def _fields(t):
    return [t.domain, t.user, t.start, t.rows, t.row, t.score]


def _same(a, b):
    for x, y in zip(a, b):
        x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        y = y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        if x.shape != y.shape or not np.array_equal(x.astype(np.int64), y.astype(np.int64)):
            return False
    return True


def run(rows, domains, users, items, k, with_item, reps, warmup, dev):
    rng = np.random.default_rng(0)
    score = rng.random(rows).astype(np.float32)
    pred = torch.from_numpy(score).to(dev)
    rng.random(rows)                                                            # rank_bench's draws: the same evaluation set
    label = torch.from_numpy((rng.random(rows) < 0.1 + 0.3 * score).astype(np.int16)).to(dev)
    X = np.zeros((rows, 4), dtype=np.int32)
    X[:, 1] = rng.integers(0, domains, size=rows)
    X[:, 2] = (rng.zipf(1.3, size=rows) - 1) % users
    X[:, 3] = rng.integers(0, items, size=rows)
    Xd = torch.from_numpy(X).to(dev)
    domain, user, item = Xd[:, 1], Xd[:, 2], (Xd[:, 3] if with_item else None)

    calls = {"eval_rank": lambda: eval_rank(pred, label, user, users, domain, domains, (k,)).ndcg.cpu(),
             "eval_topk": lambda: eval_topk(pred, user, users, domain, domains, item, k),
             "torch_ops": lambda: torch_topk(pred, user, domain, item, users, k)[2].cpu()}

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
    t = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t[name].append(timed(fn))
    res = {"rows": rows, "domains": domains, "users": users, "k": k, "items": items if with_item else None, "reps": reps}
    for name, v in t.items():
        res[name + "_ms_median"], res[name + "_ms_min"], res[name + "_ms_max"] = statistics.median(v), min(v), max(v)
    res["eval_topk_over_eval_rank"] = res["eval_topk_ms_median"] / res["eval_rank_ms_median"]
    res["eval_topk_over_torch_ops"] = res["eval_topk_ms_median"] / res["torch_ops_ms_median"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = numpy_topk(pred, user, domain, item, users, k)
    res["numpy_topk_ms"] = (time.perf_counter() - t0) * 1e3
    top = calls["eval_topk"]()
    res["device_equals_torch_ops"] = _same(_fields(top), torch_topk(pred, user, domain, item, users, k))
    res["device_equals_numpy"] = _same(_fields(top), host)
    res["groups"], res["entries"] = top.n_out.cpu().tolist()
    res["truncated_groups"] = int((top.rows > k).sum().item())
    res["err"] = int(top.err.item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--domains", type=int, nargs="+", default=[3, 50])
    ap.add_argument("--users", type=int, default=50_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bench needs a GPU")
    dev = torch.device("cuda:0")
    ok = True
    for domains in a.domains:
        for with_item in (False, True):
            res = run(a.rows, domains, a.users, a.items, a.k, with_item, a.reps, a.warmup, dev)
            print(json.dumps(res), flush=True)
            ok = ok and res["device_equals_torch_ops"] and res["device_equals_numpy"]
    if not ok:
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
