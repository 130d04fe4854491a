"""Times recommending from an item catalogue — catalog_rows, the eval forward and catalog_topk per tile — beside the route the
library offered before them, to the same lists on the same tiles: torch indexing to build the tile's rows, the same forward,
eval_topk with the item column, TopK.merge into the running lists (seen pairs scored -inf there and trimmed at the end).

Setup: PLE-3 at bench.py's dimensions (26 fields, embedding 16, experts ((256, 128), (64,)), towers (64, 32), bf16), 2 000 contexts x
20 000 items, k = 10, 50 seen items per context.  Per-tile figures are medians of 20 repetitions after a warm-up, each between two
device events with a synchronisation before and after; the select call is timed on the second item tile of a context, its lists
holding the first tile's result (restored, untimed, before every repetition), as nearly every tile of a pass finds them.
Whole-pool throughput (rows per second through Evaluator.recommend_catalog, the one read at the end included) is measured once per
tile_rows in {4096, 8192, 16384, 32768}.

Before any time is printed the lists of both routes over the WHOLE pool are compared, item ids and score bits; the run aborts
when they differ.  Needs a GPU: there is no fallback.  Prints JSON lines; no threshold."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.evaluate import CatalogTopK, Evaluator, TopK, catalog_rows, catalog_seen, catalog_topk, eval_topk  # noqa: E402
from cdcmdr_amd.model.ple import PLE  # noqa: E402

DOMAIN_COL, N_DOMAIN = 10, 3
ITEM_COLS = [1, 2, 3]                                   # catalogue column 0, the item id, goes to column 1 of X


def torch_rows(context, catalog, u0, ub, i0, ib):
    """the tile by torch indexing, and the tile's context index per row"""
    X = context[u0:u0 + ub].repeat_interleave(ib, 0)
    X[:, ITEM_COLS] = catalog[i0:i0 + ib].repeat(ub, 1)
    user = torch.arange(u0, u0 + ub, dtype=torch.int32, device=X.device).repeat_interleave(ib)
    return X, user


def forward(model, X, d2g):
    return model(X).gather(1, d2g[X[:, DOMAIN_COL].long()].reshape(-1, 1)).reshape(-1).to(torch.float32)


def old_select(pred, user, item, seen_keys, U, k):
    """eval_topk over one tile, the tile's seen pairs scored -inf"""
    keys = (user.to(torch.int64) << 32) | item.to(torch.int64)
    at = torch.searchsorted(seen_keys, keys).clamp(max=seen_keys.numel() - 1)
    pred = torch.where(seen_keys[at] == keys, torch.full_like(pred, -math.inf), pred)
    return eval_topk(pred, user, U, None, 1, item, k)


def old_route(model, context, catalog, d2g, seen_keys, k, ub, ib):
    """the whole pool through the old route -> {u: [(item, score bits)]} with the -inf entries trimmed"""
    U, I = context.shape[0], catalog.shape[0]
    acc = None
    for u0 in range(0, U, ub):
        for i0 in range(0, I, ib):
            nu, ni = min(ub, U - u0), min(ib, I - i0)
            X, user = torch_rows(context, catalog, u0, nu, i0, ni)
            top = old_select(forward(model, X, d2g), user, X[:, ITEM_COLS[0]], seen_keys, U, k)
            acc = top if acc is None else TopK.merge(acc, top, k)
    usr, start = acc.user.cpu().tolist(), acc.start.cpu().tolist()
    item, score = acc.item.cpu().numpy(), acc.score.cpu().numpy()
    out = {}
    for j, u in enumerate(usr):
        keep = score[start[j]:start[j + 1]] != -np.inf
        out[u] = list(zip(item[start[j]:start[j + 1]][keep].tolist(), score[start[j]:start[j + 1]][keep].view(np.uint32).tolist()))
    return out


def new_lists(state):
    n, item, score = state.n.cpu().tolist(), state.item.cpu().numpy(), state.score.cpu().numpy().view(np.uint32)
    return {u: list(zip(item[u, :n[u]].tolist(), score[u, :n[u]].tolist())) for u in range(len(n))}


def timed(fn, before=None):
    if before is not None:
        before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps, warmup, before=None):
    for _ in range(warmup):
        timed(fn, before)
    return statistics.median(timed(fn, before) for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=2000)
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seen", type=int, default=50)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--embed-dim", type=int, default=16)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--tile-rows", type=int, nargs="+", default=[4096, 8192, 16384, 32768])
    ap.add_argument("--tile", type=int, default=8192, help="tile_rows of the per-tile figures")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("catalog_bench needs a GPU")
    dev = torch.device("cuda:0")
    U, I, k = a.contexts, a.items, a.k
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    model = PLE([a.vocab] * a.fields, a.embed_dim, 3, 2, 2, ((256, 128), (64,)), (64, 32), 0.2).to(dev).set_precision(a.precision)
    model.eval()
    ctx = rng.integers(0, a.vocab, size=(U, a.fields)).astype(np.int32)
    ctx[:, DOMAIN_COL] = rng.integers(0, N_DOMAIN, size=U)
    cat = rng.integers(0, a.vocab, size=(I, len(ITEM_COLS))).astype(np.int32)
    cat[:, 0] = rng.permutation(a.vocab)[:I]
    context, catalog = torch.from_numpy(ctx).to(dev), torch.from_numpy(cat).to(dev)
    d2g_list = [0, 1, 2]
    d2g = torch.tensor(d2g_list, dtype=torch.int64, device=dev)
    seen_ctx = np.repeat(np.arange(U), a.seen)
    seen_item = cat[rng.integers(0, I, size=U * a.seen), 0]
    seen = tuple(t.to(dev) for t in catalog_seen(torch.from_numpy(seen_ctx), torch.from_numpy(seen_item.astype(np.int64)), U))
    seen_keys = torch.sort((torch.from_numpy(seen_ctx).to(dev) << 32) | torch.from_numpy(seen_item.astype(np.int64)).to(dev))[0]
    ev = Evaluator(model, mode="multi", domain_idx=DOMAIN_COL, n_domain=N_DOMAIN)

    with torch.no_grad():
        # agreement over the whole pool, before any time is printed
        state = ev.recommend_catalog(context, catalog, ITEM_COLS, k=k, seen=seen, domain2group=d2g_list, tile_rows=a.tile)
        got = new_lists(state)
        ib = min(I, a.tile)
        ub = max(1, a.tile // ib)
        want = old_route(model, context, catalog, d2g, seen_keys, k, ub, ib)
        differ = [u for u in range(U) if got[u] != want.get(u, [])]
        if differ:
            sys.exit(f"the routes disagree in {len(differ)} of {U} lists, first context {differ[0]}: {got[differ[0]]} != {want.get(differ[0])}")
        print(json.dumps({"agreement": "both routes give the same lists, item ids and score bits", "lists": U, "entries": sum(map(len, got.values())),
                          "contexts": U, "items": I, "k": k, "seen_per_context": a.seen, "tile_rows": a.tile, "precision": a.precision}), flush=True)

        # per-tile figures: context 0's first item tile fills the lists, the second is timed
        i1 = ib if 2 * ib <= I else 0
        box = {}
        t_rows = median_ms(lambda: box.update(X=catalog_rows(context, catalog, ITEM_COLS, 0, ub, i1, ib, d2g, DOMAIN_COL)), a.reps, a.warmup)
        X, group, _ = box["X"]
        t_fwd = median_ms(lambda: box.update(p=model(X).gather(1, group.reshape(-1, 1)).reshape(-1).to(torch.float32)), a.reps, a.warmup)
        pred = box["p"]
        first = CatalogTopK.empty(U, k, dev)
        X0, g0, _ = catalog_rows(context, catalog, ITEM_COLS, 0, ub, 0, ib, d2g, DOMAIN_COL)
        catalog_topk(first, model(X0).gather(1, g0.reshape(-1, 1)).reshape(-1).to(torch.float32), catalog, 0, ub, 0, ib, seen)
        work = CatalogTopK.empty(U, k, dev)

        def restore(src):
            def go():
                for f in ("item", "cat", "score", "n"):
                    getattr(work, f).copy_(getattr(src, f))
            return go
        t_topk = median_ms(lambda: catalog_topk(work, pred, catalog, 0, ub, i1, ib, seen), a.reps, a.warmup, restore(first))
        t_topk_cold = median_ms(lambda: catalog_topk(work, pred, catalog, 0, ub, i1, ib, seen), a.reps, a.warmup, restore(CatalogTopK.empty(U, k, dev)))
        t_build = median_ms(lambda: box.update(o=torch_rows(context, catalog, 0, ub, i1, ib)), a.reps, a.warmup)
        Xo, user = box["o"]
        t_sel = median_ms(lambda: box.update(t=old_select(pred, user, Xo[:, ITEM_COLS[0]], seen_keys, U, k)), a.reps, a.warmup)
        top1 = box["t"]
        top0 = old_select(forward(model, X0, d2g), torch.arange(0, ub, dtype=torch.int32, device=dev).repeat_interleave(ib), X0[:, ITEM_COLS[0]],
                          seen_keys, U, k)
        t_merge = median_ms(lambda: TopK.merge(top0, top1, k), a.reps, a.warmup)
        new_pair, old_trio = t_rows + t_topk, t_build + t_sel + t_merge
        print(json.dumps({"tile": [ub, ib], "reps": a.reps, "catalog_rows_ms": t_rows, "forward_ms": t_fwd, "catalog_topk_ms": t_topk,
                          "catalog_topk_empty_lists_ms": t_topk_cold, "torch_rows_ms": t_build, "eval_topk_with_seen_mask_ms": t_sel,
                          "topk_merge_ms": t_merge, "new_rows_plus_topk_ms": new_pair, "old_rows_plus_topk_plus_merge_ms": old_trio,
                          "new_over_old": new_pair / old_trio, "forward_share_of_new_tile": t_fwd / (t_fwd + new_pair),
                          "forward_share_of_old_tile": t_fwd / (t_fwd + old_trio)}), flush=True)

        # whole-pool throughput; the first pass at a tile size builds the forward's plans for its batch sizes
        for tile_rows in a.tile_rows:
            ev.recommend_catalog(context[:4], catalog, ITEM_COLS, k=k, seen=(seen[0][:5], seen[1]), domain2group=d2g_list, tile_rows=tile_rows)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.recommend_catalog(context, catalog, ITEM_COLS, k=k, seen=seen, domain2group=d2g_list, tile_rows=tile_rows)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"tile_rows": tile_rows, "pool_rows": U * I, "seconds": dt, "rows_per_second": U * I / dt}), flush=True)


if __name__ == "__main__":
    main()
