"""Recommending from an item catalogue in plain Python (helper of tests/test_catalog_cpu.py and tests/test_gpu_catalog.py; not a test).

cdc_catalog_topk's contract (include/cdcmdr.h) restated with `sorted`:

  context    one request, row u of `context` int32 [U, F]: the model's full id row with the user side and the domain filled in.
  catalogue  `catalog` int32 [I, C]; item_cols names the C distinct columns of X its columns overwrite; column 0 is the item id, which
             must be >= 0 and distinct over the catalogue.
  pool       pool row (u, i) is context u with X[item_cols[c]] = catalog[i, c] (`pool_rows`).  One list per context; contexts are
             never grouped: two contexts of one user are two lists.
  excluded   candidate (u, i) is left out silently when catalog[i, 0] is in context u's seen set (duplicates and ids that are not in
             the catalogue are allowed there).  It is left out and REPORTED when its score is NaN or its item id is negative, seen or
             not: the error word is 1 + the largest such context index, 0 when there is none.
  order      inside a list the key (-(s + 0.0), item, catalogue row): descending score with -0.0 and +0.0 as one score, then ascending
             item id, then ascending catalogue row (which only matters when ids repeat; it keeps the order total).
  result     per context n = min(k, survivors) entries (item, catalogue row, score), best first; laid out as the device does (`dense`)
             the entries past n are -1, -1 and the NaN 0x7fc00000.  1 <= k <= 1024.
  running    `fold_exact` replaces every context's list of a tile by the first k, in that order, of (old list + the tile's candidates
             that are not excluded); folding disjoint item tiles in any order and with any shapes gives `catalog_exact`'s result.
"""
import math

import numpy as np

MAX_K = 1024
PAD_SCORE = 0x7fc00000


def _key(e):
    item, cat, s = e
    return (-(float(s) + 0.0), item, cat)


def _seen_of(seen, u):
    if seen is None:
        return ()
    return seen.get(u, ()) if isinstance(seen, dict) else seen[u]


def fold_exact(lists, err, score, ids, k, u0=0, i0=0, seen=None):
    """lists: one list of (item, catalogue row, score float32) per context, all U of them; score [Ub][Ib]: the tile's scores, contexts
    u0.., catalogue rows i0..; ids: the WHOLE catalogue's id column; seen: None, {u: ids} or a sequence indexed by u.
    -> (new lists, new error word); the inputs are left as they are."""
    assert 1 <= k <= MAX_K
    score = np.asarray(score, dtype=np.float32)
    out = [list(l) for l in lists]
    for a in range(score.shape[0]):
        u = u0 + a
        gone = set(int(v) for v in _seen_of(seen, u))
        cand = []
        for b in range(score.shape[1]):
            item, s = int(ids[i0 + b]), score[a, b]
            if math.isnan(float(s)) or item < 0:
                err = max(err, u + 1)
            elif item not in gone:
                cand.append((item, i0 + b, s))
        out[u] = sorted(out[u] + cand, key=_key)[:k]
    return out, err


def catalog_exact(score, ids, k, seen=None):
    """score [U][I], ids [I] -> (lists, err): every context's first k candidates in one pass over all items"""
    score = np.asarray(score, dtype=np.float32)
    return fold_exact([[] for _ in range(score.shape[0])], 0, score, ids, k, 0, 0, seen)


def dense(result, k):
    """-> dict of numpy arrays laid out as cdc_catalog_topk's state: item, cat int32 [U, k], score uint32 bits [U, k], n int32 [U], err"""
    lists, err = result
    U = len(lists)
    item, cat = np.full((U, k), -1, dtype=np.int32), np.full((U, k), -1, dtype=np.int32)
    score = np.full((U, k), PAD_SCORE, dtype=np.uint32)
    for u, l in enumerate(lists):
        for j, (it, c, s) in enumerate(l):
            item[u, j], cat[u, j] = it, c
            score[u, j] = np.asarray(s, dtype=np.float32).view(np.uint32)
    return {"item": item, "cat": cat, "score": score, "n": np.array([len(l) for l in lists], dtype=np.int32), "err": err}


def pool_rows(context, catalog, item_cols, u0=0, ub=None, i0=0, ib=None):
    """the tile of pool rows as an int32 [ub * ib, F] array: row (u - u0) * ib + (i - i0)"""
    context, catalog = np.asarray(context), np.asarray(catalog)
    ub = context.shape[0] - u0 if ub is None else ub
    ib = catalog.shape[0] - i0 if ib is None else ib
    X = np.repeat(context[u0:u0 + ub], ib, axis=0).astype(np.int32)
    for c, f in enumerate(item_cols):
        X[:, f] = np.tile(catalog[i0:i0 + ib, c], ub)
    return X


# the hand example of INTEGRATION.md: 3 contexts x 5 items, k = 2
HAND_IDS = [7, 3, 9, 4, 8]
HAND_SCORE = [[0.5, 0.9, 0.9, -0.0, 0.1],
              [0.0, -0.0, math.nan, 0.0, 0.0],
              [0.2, 0.3, 0.4, 0.5, 0.6]]
HAND_SEEN = {0: [3], 2: [3, 4, 8, 9, 100]}
HAND_K = 2
# context 0: item 3 is seen; 0.9 -> item 9 (row 2), then 0.5 -> item 7 (row 0)
# context 1: the NaN candidate is reported (error word 2); the zeros tie whatever their sign -> item 3 (row 1, -0.0), item 4 (row 3)
# context 2: everything but item 7 is seen: one entry, then padding
HAND_LISTS = [[(9, 2, 0.9), (7, 0, 0.5)], [(3, 1, -0.0), (4, 3, 0.0)], [(7, 0, 0.2)]]
HAND_ERR = 2
