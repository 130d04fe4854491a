"""Recommending from an item catalogue, the parts that need no GPU: the plain-Python restatement (tests/catalog_exact.py) against
tests/topk_exact.py on the materialised pool, tile folding, the documented hand example, `catalog_seen`, and the argument checks of
cdc_catalog_rows / cdc_catalog_topk / Evaluator.recommend_catalog, none of which touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from catalog_exact import (HAND_ERR, HAND_IDS, HAND_K, HAND_LISTS, HAND_SCORE, HAND_SEEN, PAD_SCORE, catalog_exact, dense, fold_exact,
                           pool_rows)
from topk_exact import topk_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(lists):
    return [[(it, c, np.asarray(s, dtype=np.float32).view(np.uint32).item()) for it, c, s in l] for l in lists]


def _ties(rng, U, I, levels=8):
    """scores on a coarse grid with both zeros: heavy ties"""
    s = (rng.integers(-levels, levels + 1, size=(U, I)) / levels).astype(np.float32)
    s[rng.random((U, I)) < 0.1] = -0.0
    return s


def _seen(rng, U, ids, share=0.3):
    return {u: sorted(rng.choice(ids, size=int(share * len(ids)), replace=True).tolist() + [10 ** 6 + u]) for u in range(0, U, 2)}


@pytest.mark.parametrize("k", [1, 3, 50])
def test_restatement_equals_topk_exact_on_the_materialised_pool(k):
    rng = np.random.default_rng(k)
    U, I = 7, 23
    ids = rng.permutation(100)[:I]
    for s in (rng.random((U, I)).astype(np.float32), _ties(rng, U, I)):
        lists, err = catalog_exact(s, ids, k)
        groups, _, want, werr = topk_exact(s.reshape(-1), np.repeat(np.arange(U), I), U, None, 1, np.tile(ids, U), k)
        assert err == 0 and werr == 0 and groups == [(0, u) for u in range(U)]
        got = [[(it, sc.view(np.uint32).item()) for it, _, sc in l] for l in lists]
        ref = [[(int(ids[r % I]), sc.view(np.uint32).item()) for r, sc in l] for l in want]
        assert got == ref
        assert all(c == int(np.nonzero(ids == it)[0][0]) for l in lists for it, c, _ in l)


def test_fold_over_any_split_equals_the_one_shot_result():
    rng = np.random.default_rng(11)
    U, I, k = 5, 61, 6
    ids = rng.permutation(500)[:I]
    s = _ties(rng, U, I)
    s[1, 7] = s[4, 60] = np.nan
    for seen in (None, _seen(rng, U, ids)):
        want = catalog_exact(s, ids, k, seen)
        assert want[1] == 5
        for ub, ib in ((1, 1), (2, 7), (5, 20), (3, 61), (5, 60)):
            for reverse in (False, True):
                lists, err = [[] for _ in range(U)], 0
                i_tiles = list(range(0, I, ib))[::-1] if reverse else list(range(0, I, ib))
                for u0 in range(0, U, ub):
                    for i0 in i_tiles:
                        lists, err = fold_exact(lists, err, s[u0:u0 + ub, i0:i0 + ib], ids, k, u0, i0, seen)
                assert _bits(lists) == _bits(want[0]) and err == want[1], (ub, ib, reverse)
    # repeated ids break the precondition; the catalogue row keeps the order total, and folding still equals the one-shot result
    ids2 = ids.copy()
    ids2[10:20] = ids2[0]
    want = catalog_exact(s, ids2, k)
    lists, err = [[] for _ in range(U)], 0
    for i0 in (40, 0, 20):
        lists, err = fold_exact(lists, err, s[:, i0:i0 + 20 + (i0 == 40)], ids2, k, 0, i0)
    assert _bits(lists) == _bits(want[0])


def test_the_hand_example_of_the_docs():
    got = catalog_exact(HAND_SCORE, HAND_IDS, HAND_K, HAND_SEEN)
    assert _bits(got[0]) == _bits(HAND_LISTS) and got[1] == HAND_ERR
    d = dense(got, HAND_K)
    assert d["n"].tolist() == [2, 2, 1] and d["item"].tolist() == [[9, 7], [3, 4], [7, -1]] and d["cat"].tolist() == [[2, 0], [1, 3], [0, -1]]
    assert d["score"][2, 1] == PAD_SCORE and d["score"][1, 0] == 0x80000000          # the -0.0 is bit-copied
    # a negative id is reported for every context and leaves only its own candidates out
    got = catalog_exact(HAND_SCORE, [7, -3, 9, 4, 8], 5)
    assert got[1] == 3 and [[it for it, _, _ in l] for l in got[0]] == [[9, 7, 8, 4], [4, 7, 8], [8, 4, 9, 7]]
    X = pool_rows([[5, 0, 0, 1], [6, 0, 0, 2]], [[10, 7], [11, 8], [12, 9]], [2, 1], 0, 2, 1, 2)
    assert X.tolist() == [[5, 8, 11, 1], [5, 9, 12, 1], [6, 8, 11, 2], [6, 9, 12, 2]]


def test_catalog_seen_against_a_dict():
    from cdcmdr_amd.evaluate import catalog_seen
    rng = np.random.default_rng(2)
    U, n = 9, 300
    ctx, item = rng.integers(0, U - 1, size=n), rng.integers(-5, 40, size=n)          # context U - 1 has an empty slice
    want = {u: sorted(item[ctx == u].tolist()) for u in range(U)}
    start, seen = catalog_seen(torch.from_numpy(ctx), torch.from_numpy(item), U)
    assert start.dtype == torch.int32 and seen.dtype == torch.int32 and start.numel() == U + 1 and seen.numel() == n
    st, se = start.tolist(), seen.tolist()
    assert st[0] == 0 and st[U] == n and {u: se[st[u]:st[u + 1]] for u in range(U)} == want
    start, seen = catalog_seen(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3)
    assert start.tolist() == [0, 0, 0, 0] and seen.numel() == 0
    with pytest.raises(ValueError, match="outside"):
        catalog_seen([0, 3], [1, 2], 3)
    with pytest.raises(ValueError, match="context indices"):
        catalog_seen([0, 1], [1], 3)


def test_catalog_limits_match_the_header():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import CATALOG_MAX_K
    import catalog_exact as E
    src = open(os.path.join(ROOT, "include", "cdcmdr.h")).read()
    for macro, val in (("CDC_CATALOG_MAX_K", _lib.CATALOG_MAX_K), ("CDC_CATALOG_MAX_F", _lib.CATALOG_MAX_F)):
        m = re.search(rf"#define\s+{macro}\s+(\d+)", src)
        assert m and int(m.group(1)) == val, macro
    assert CATALOG_MAX_K == _lib.CATALOG_MAX_K == E.MAX_K


def test_cdc_catalog_calls_refuse_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, never dereferenced on the host
    cols = (C.c_int32 * 2)(3, 1)

    def rows(context=p, ld_context=6, U=10, catalog=p, ld_catalog=2, I=20, item_cols=cols, n_cols=2, F=6, u0=0, ub=10, i0=0, ib=20, X=p,
             group=None, g_of_d=None, n_domain=0, domain_col=-1, domain=None):
        return lib.cdc_catalog_rows(context, ld_context, U, catalog, ld_catalog, I, item_cols, n_cols, F, u0, ub, i0, ib, X, group, g_of_d,
                                    n_domain, domain_col, domain, None, None)

    def topk(score=p, ids=p, ld=2, U=10, I=20, u0=0, ub=10, i0=0, ib=20, seen_start=None, seen_item=None, n_seen=0, k=10, item=p, cat=p, out=p,
             n=p):
        return lib.cdc_catalog_topk(score, ids, ld, U, I, u0, ub, i0, ib, seen_start, seen_item, n_seen, k, item, cat, out, n, None, None)

    for kw in ({"context": None}, {"catalog": None}, {"item_cols": None}, {"X": None}):
        assert rows(**kw) == -1 and b"catalog_rows: null pointer" in lib.cdc_last_error(), kw
    for kw in ({"score": None}, {"ids": None}, {"item": None}, {"cat": None}, {"out": None}, {"n": None}):
        assert topk(**kw) == -1 and b"catalog_topk: null pointer" in lib.cdc_last_error(), kw
    for k in (0, -1, 1025, 1 << 30):
        assert topk(k=k) == -1 and b"lies outside [1, 1024]" in lib.cdc_last_error(), k
    for call, name in ((rows, b"catalog_rows"), (topk, b"catalog_topk")):
        assert call(ub=1 << 16, ib=1 << 15, U=1 << 20, I=1 << 20) == -1 and name + b": a tile of 65536 x 32768 rows reaches 2^31" == lib.cdc_last_error()
        for kw in ({"u0": -1}, {"u0": 1}, {"ub": 0}, {"ub": 11}, {"i0": -1}, {"i0": 1}, {"ib": 0}, {"ib": 21}, {"u0": 10, "ub": 1}, {"i0": 20, "ib": 1},
                   {"u0": (1 << 62), "ub": 1}):
            assert call(**kw) == -1 and name + b": tile [" in lib.cdc_last_error() and b"lies outside [0, 10) x [0, 20)" in lib.cdc_last_error(), kw
        for kw in ({"U": 0, "u0": 0, "ub": 1}, {"I": 0}, {"U": 1 << 31}, {"I": 1 << 31}):
            assert call(**kw) == -1 and name + b": bad sizes U=" in lib.cdc_last_error(), kw
    for bad, text in (((6, 1), b"item_cols[0]=6 lies outside [0, 6)"), ((3, -1), b"item_cols[1]=-1 lies outside [0, 6)"),
                      ((3, 3), b"item_cols[1]=3 repeats column 3")):
        assert rows(item_cols=(C.c_int32 * 2)(*bad)) == -1 and text in lib.cdc_last_error(), bad
    for kw in ({"F": 0}, {"F": 257, "ld_context": 300}, {"n_cols": 0}, {"n_cols": 7}, {"ld_context": 5}, {"ld_catalog": 1}):
        assert rows(**kw) == -1 and b"catalog_rows: bad sizes F=" in lib.cdc_last_error(), kw
    assert rows(group=p, g_of_d=p, n_domain=3, domain_col=6) == -1 and b"domain_col=6 lies outside [0, 6)" in lib.cdc_last_error()
    assert rows(domain=p, domain_col=-1) == -1 and b"domain_col=-1" in lib.cdc_last_error()
    assert rows(group=p, domain_col=2) == -1 and rows(group=p, g_of_d=p, n_domain=0, domain_col=2) == -1 and b"group_of_domain" in lib.cdc_last_error()
    assert topk(seen_start=p) == -1 and topk(seen_item=p) == -1 and topk(n_seen=5) == -1 and b"the seen set" in lib.cdc_last_error()
    assert topk(seen_start=p, seen_item=p, n_seen=-1) == -1 and topk(seen_start=p, seen_item=p, n_seen=1 << 31) == -1
    assert topk(ld=0) == -1 and b"ld_catalog" in lib.cdc_last_error()


def test_catalog_host_mirror_checks_arguments():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import CatalogTopK, Evaluator, catalog_rows, catalog_topk
    context = torch.zeros((4, 5), dtype=torch.int32)
    catalog = torch.arange(12, dtype=torch.int32).reshape(6, 2)
    ev = Evaluator(None, mode="single")
    for k in (0, 1025, -1, 2.5, True):
        with pytest.raises(ValueError, match="k="):
            ev.recommend_catalog(context, catalog, [1, 2], k=k)
    rep = catalog.clone()
    rep[4, 0] = rep[1, 0]
    with pytest.raises(ValueError, match="repeats an item id"):
        ev.recommend_catalog(context, rep, [1, 2])
    neg = catalog.clone()
    neg[3, 0] = -7
    with pytest.raises(ValueError, match="negative item id"):
        ev.recommend_catalog(context, neg, [1, 2])
    with pytest.raises(ValueError, match="domain2group"):
        Evaluator(None, mode="multi", domain_idx=4, n_domain=3).recommend_catalog(context, catalog, [1, 2])
    with pytest.raises(ValueError, match="domain2group"):
        Evaluator(None, mode="multi").recommend_catalog(context, catalog, [1, 2], domain2group=[0, 1, 2])
    with pytest.raises(ValueError, match="tile_rows"):
        ev.recommend_catalog(context, catalog, [1, 2], tile_rows=0)
    with pytest.raises(_lib.HipExtensionError):                 # every check passed: the pool itself needs the device
        ev.recommend_catalog(context, catalog, [1, 2])
    with pytest.raises(_lib.HipExtensionError):
        catalog_rows(context, catalog, [1, 2], 0, 4, 0, 6)
    with pytest.raises(_lib.HipExtensionError):
        catalog_topk(CatalogTopK.empty(4, 3, "cpu"), torch.zeros(24), catalog, 0, 4, 0, 6)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k="):
            CatalogTopK.empty(4, k, "cpu")
    st = CatalogTopK.empty(2, 3, "cpu")
    assert st.item.tolist() == [[-1] * 3] * 2 and st.cat.tolist() == [[-1] * 3] * 2 and bool(torch.isnan(st.score).all())
    assert st.n.tolist() == [0, 0] and st.k == 3 and st.err.tolist() == [0] and st.lists() == {0: ([], []), 1: ([], [])}
    st.n[1], st.item[1, 0], st.score[1, 0] = 1, 8, 0.25
    assert st.lists() == {0: ([], []), 1: ([8], [0.25])}
