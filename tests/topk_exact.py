"""The per-user top-K lists in plain Python (helper of tests/test_topk_cpu.py and tests/test_gpu_topk.py; not a test).

cdc_eval_topk's contract restated with a dict and `sorted`:

  group     a row's group is (domain, user); domain is 0 throughout when there is no domain column.
  excluded  a row with a NaN score, a user outside [0, n_user), a domain outside [0, n_domain) or (with items) a negative item is in
            no list; the error word is 1 + the largest index of such a row, 0 when there is none.
  order     inside a group the key (-(s + 0.0), item, row): descending score with -0.0 and +0.0 as one score, then ascending item
            (0 for every row when there are no items), then ascending row index.  A total order.
  de-dup    with items, walking a group in that order, a row whose item has been seen is dropped.
  cut       the first min(k, survivors) rows.

`topk_exact` returns the groups in ascending (domain, user) order, each group's survivor count before the cut, the lists and the
error word; `flat` lays them out as the device does; `merge_exact` restates TopK.merge on such results.
"""
import math

import numpy as np


def topk_exact(s, u, n_user, dom=None, n_domain=1, item=None, k=10):
    """-> (groups [(domain, user)], survivors [int], lists [[(row, score float32)]], err)"""
    s = np.asarray(s, dtype=np.float32)
    u = np.asarray(u).astype(np.int64)
    n = len(s)
    d = np.zeros(n, dtype=np.int64) if dom is None else np.asarray(dom).astype(np.int64)
    it = None if item is None else np.asarray(item).astype(np.int64)
    by_group, err = {}, 0
    for i in range(n):
        bad = math.isnan(float(s[i])) or not 0 <= u[i] < n_user or not 0 <= d[i] < n_domain or (it is not None and it[i] < 0)
        if bad:
            err = i + 1                                                    # ascending i: the largest stays
            continue
        by_group.setdefault((int(d[i]), int(u[i])), []).append(i)
    groups, survivors, lists = [], [], []
    for g in sorted(by_group):
        rows = sorted(by_group[g], key=lambda i: (-(float(s[i]) + 0.0), 0 if it is None else int(it[i]), i))
        if it is not None:
            seen, kept = set(), []
            for i in rows:
                if int(it[i]) not in seen:
                    seen.add(int(it[i]))
                    kept.append(i)
            rows = kept
        groups.append(g)
        survivors.append(len(rows))
        lists.append([(i, s[i]) for i in rows[:k]])
    return groups, survivors, lists, min(err, 0x7fffffff)


def flat(result):
    """-> dict of numpy arrays laid out as cdc_eval_topk's outputs: domain, user, start [G + 1], rows, row, score (as uint32 bits)"""
    groups, survivors, lists, err = result
    start = np.cumsum([0] + [len(l) for l in lists])
    return {"domain": np.array([g[0] for g in groups], dtype=np.int32), "user": np.array([g[1] for g in groups], dtype=np.int32),
            "start": start.astype(np.int32), "rows": np.array(survivors, dtype=np.int32),
            "row": np.array([r for l in lists for r, _ in l], dtype=np.int32),
            "score": np.array([v for l in lists for _, v in l], dtype=np.float32).view(np.uint32), "err": err}


def merge_exact(a, b, n_user, n_domain, item_a=None, item_b=None, k=10, row_offset=0):
    """TopK.merge on two `topk_exact` results: the entries of a, then those of b, ranked again under the same rules; the rows of the
    result are a's row indices and b's shifted by row_offset.  item_a / item_b: the item column of each INPUT (indexed by row)."""
    s, u, d, it, orig = [], [], [], [], []
    for (groups, _, lists, _), items, off in ((a, item_a, 0), (b, item_b, row_offset)):
        for g, l in zip(groups, lists):
            for r, v in l:
                s.append(v)
                d.append(g[0])
                u.append(g[1])
                orig.append(r + off)
                if items is not None:
                    it.append(int(items[r]))
    groups, survivors, lists, _ = topk_exact(np.array(s, dtype=np.float32), u, n_user, d, n_domain, it if it else None, k)
    return groups, survivors, [[(orig[p], v) for p, v in l] for l in lists], 0
