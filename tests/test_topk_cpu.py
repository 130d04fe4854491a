"""CPU-only checks of the per-user top-K lists: the pure-Python helper (tests/topk_exact.py) on a hand-worked example, on its two
properties and on every rule of the contract, TopK.merge's semantics on the helper, and the argument checks of cdc_eval_topk,
eval_topk and Evaluator.recommend, which come before anything touches a device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from rank_exact import rank_exact
from topk_exact import flat, merge_exact, topk_exact

#        row:   0    1    2    3     4    5    6    7    8
DOM = [0, 0, 0, 0, 1, 1, 0, 0, 1]
USER = [1, 1, 1, 1, 0, 0, 0, 1, 0]
ITEM = [5, 5, 7, 3, 2, 1, 9, 7, 2]
SCORE = [0.5, 0.9, 0.9, 0.1, -0.0, 0.0, 0.3, 0.9, 0.0]


def _rows(result):
    return [[r for r, _ in l] for l in result[2]]


def test_hand_example():
    # with items, per domain, k = 2.  (0, 1): 0.9 three times -> item 5 (row 1), item 7 (rows 2 and 7: row 2 survives), then 0.5 of item 5
    # (a repeat), then item 3: survivors 1, 2, 3.  (1, 0): three zeros of either sign tie -> item 1 (row 5), item 2 (row 4 before row 8).
    got = topk_exact(SCORE, USER, 2, DOM, 2, ITEM, 2)
    assert got[0] == [(0, 0), (0, 1), (1, 0)] and got[1] == [1, 3, 2] and _rows(got) == [[6], [1, 2], [5, 4]] and got[3] == 0
    f = flat(got)
    assert f["start"].tolist() == [0, 1, 3, 5] and f["row"].tolist() == [6, 1, 2, 5, 4] and f["rows"].tolist() == [1, 3, 2]
    assert f["score"].tolist() == np.array([0.3, 0.9, 0.9, 0.0, -0.0], dtype=np.float32).view(np.uint32).tolist()   # bit copies: row 4 is -0.0
    # without items every row is a candidate and equal scores go by row index
    got = topk_exact(SCORE, USER, 2, DOM, 2, None, 2)
    assert got[1] == [1, 5, 3] and _rows(got) == [[6], [1, 2], [4, 5]]
    # all rows by user, items, k above every group: full rankings.  user 0: 0.3, then the zeros by item
    got = topk_exact(SCORE, USER, 2, None, 1, ITEM, 10)
    assert got[0] == [(0, 0), (0, 1)] and got[1] == [3, 3] and _rows(got) == [[6, 5, 4], [1, 2, 3]]


def _figures_from_lists(result, y, s, u, dom, K):
    """precision, recall and hit rate at K of every group with a positive, averaged: exact rationals from the lists alone"""
    y = np.asarray(y)
    d = np.zeros(len(y), dtype=np.int64) if dom is None else np.asarray(dom)
    sums, counted = [Fraction(0)] * 3, 0
    for (gd, gu), l in zip(result[0], result[2]):
        P = int(y[(d == gd) & (np.asarray(u) == gu)].sum())
        if P == 0:
            continue
        hits = sum(int(y[r]) for r, _ in l[:K])
        counted += 1
        sums = [sums[0] + Fraction(hits, K), sums[1] + Fraction(hits, P), sums[2] + (1 if hits else 0)]
    return [v / counted for v in sums], counted


def test_lists_reproduce_rank_exact_on_tie_free_scores():
    from cdcmdr_amd.evaluate import rank_discounts
    rng = np.random.default_rng(11)
    n, n_user, n_domain, ks = 1500, 60, 3, (1, 5, 10)
    s = (rng.permutation(n) / n).astype(np.float32)
    assert len(set(s.tolist())) == n
    y, u, dom = rng.integers(0, 2, size=n), rng.integers(0, n_user, size=n), rng.integers(0, n_domain, size=n)
    vals, counted = rank_exact(y, s, u, dom, n_domain, ks, rank_discounts(10).numpy())[:2]
    per_domain = topk_exact(s, u, n_user, dom, n_domain, None, 10)
    by_user = topk_exact(s, u, n_user, None, 1, None, 10)
    for q, K in enumerate(ks):
        for d in range(n_domain + 1):
            if d < n_domain:
                keep = [j for j, g in enumerate(per_domain[0]) if g[0] == d]
                res = ([per_domain[0][j] for j in keep], None, [per_domain[2][j] for j in keep], 0)
                figs, c = _figures_from_lists(res, y, s, u, dom, K)
            else:
                figs, c = _figures_from_lists(by_user, y, s, u, None, K)
            assert c == counted[d]
            assert figs == [vals[d]["precision"][q], vals[d]["recall"][q], vals[d]["hit"][q]], (K, d)


def _heavy_ties(rng, n, n_user, n_domain):
    s = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.5, 0.75, 1.0, -1.0, 2.0], dtype=np.float32), size=n)
    return s, rng.integers(0, n_user, size=n), rng.integers(0, n_domain, size=n), rng.integers(0, 12, size=n)


def _as_sequences(result, item):
    """the lists as (domain, user) -> [(item, score with -0.0 folded)] and the survivor counts: what must not depend on the row order"""
    return {g: [(int(item[r]), float(v) + 0.0) for r, v in l] for g, l in zip(result[0], result[2])}, dict(zip(result[0], result[1]))


def test_item_lists_do_not_depend_on_the_row_order():
    rng = np.random.default_rng(12)
    n, n_user, n_domain = 2000, 40, 3
    s, u, dom, item = _heavy_ties(rng, n, n_user, n_domain)
    want = _as_sequences(topk_exact(s, u, n_user, dom, n_domain, item, 5), item)
    for _ in range(3):
        p = rng.permutation(n)
        assert _as_sequences(topk_exact(s[p], u[p], n_user, dom[p], n_domain, item[p], 5), item[p]) == want
    seqs = want[0]
    assert any(len(l) == 5 for l in seqs.values()) and all(len({i for i, _ in l}) == len(l) for l in seqs.values())   # no item twice


def test_k_beyond_every_group_returns_full_rankings():
    rng = np.random.default_rng(13)
    s, u, dom, item = _heavy_ties(rng, 300, 9, 2)
    for it in (None, item):
        full = topk_exact(s, u, 9, dom, 2, it, 2 ** 31 - 1)
        assert [len(l) for l in full[2]] == full[1]
        if it is None:
            assert sum(full[1]) == 300
        for k in (1, 3):
            cut = topk_exact(s, u, 9, dom, 2, it, k)
            assert cut[0] == full[0] and cut[1] == full[1]
            assert _rows(cut) == [l[:k] for l in _rows(full)]


def test_signed_zeros_are_one_score():
    s = np.array([-0.0, 0.0, -0.0, 1e-30, -1e-30], dtype=np.float32)
    got = topk_exact(s, [0] * 5, 1, None, 1, None, 5)
    assert _rows(got) == [[3, 0, 1, 2, 4]]                      # the zeros in row order whatever their sign
    got = topk_exact(s, [0] * 5, 1, None, 1, [4, 2, 3, 9, 9], 5)
    assert _rows(got) == [[3, 1, 2, 0]]                         # ... and in item order with items; row 4 repeats item 9
    assert flat(got)["score"].tolist() == s[[3, 1, 2, 0]].view(np.uint32).tolist()


def test_every_exclusion_and_the_error_word():
    s = np.array([0.5, 0.4, 0.3, 0.2, 0.1, 0.6], dtype=np.float32)
    u, dom, item = [0, 0, 1, 1, 0, 1], [0, 1, 0, 1, 0, 1], [1, 2, 3, 4, 5, 6]
    assert topk_exact(s, u, 2, dom, 2, item, 9)[3] == 0
    bad = s.copy()
    bad[1] = np.nan
    got = topk_exact(bad, u, 2, dom, 2, item, 9)
    assert got[3] == 2 and got[0] == [(0, 0), (0, 1), (1, 1)] and _rows(got) == [[0, 4], [2], [5, 3]]
    got = topk_exact(s, [0, 0, 2 ** 31 - 1, 1, 0, 1], 2, dom, 2, item, 9)
    assert got[3] == 3 and all(2 not in l for l in _rows(got)) and got[0] == [(0, 0), (1, 0), (1, 1)]      # not clamped into user 1
    got = topk_exact(s, [0, 0, 1, 1, -1, 1], 2, dom, 2, item, 9)
    assert got[3] == 5 and _rows(got)[0] == [0]
    got = topk_exact(s, u, 2, [0, 1, 0, -1, 0, 1], 2, item, 9)
    assert got[3] == 4 and _rows(got) == [[0, 4], [2], [1], [5]]
    got = topk_exact(s, u, 2, [0, 1, 0, 2, 0, 1], 2, item, 9)
    assert got[3] == 4
    got = topk_exact(s, u, 2, dom, 2, [1, 2, 3, 4, 5, -5], 9)
    assert got[3] == 6 and got[0] == [(0, 0), (0, 1), (1, 0), (1, 1)] and _rows(got)[3] == [3]
    assert topk_exact(s, u, 2, dom, 2, None, 9)[3] == 0         # no item column: nothing to flag
    got = topk_exact(bad, [0, 0, 1, 1, 0, 7], 2, dom, 2, item, 9)
    assert got[3] == 6                                          # the LARGEST bad index
    got = topk_exact(np.full(3, np.nan, dtype=np.float32), [0, 0, 0], 1)
    assert got == ([], [], [], 3) and flat(got)["start"].tolist() == [0]


@pytest.mark.parametrize("with_item", [False, True])
def test_merge_of_three_passes_equals_one_call(with_item):
    rng = np.random.default_rng(14)
    n, n_user, n_domain, k = 900, 25, 3, 4
    s, u, dom, item = _heavy_ties(rng, n, n_user, n_domain)
    it = item if with_item else None
    want = topk_exact(s, u, n_user, dom, n_domain, it, k)
    cuts, acc, acc_item = [0, 250, 610, n], None, None
    for a, b in zip(cuts, cuts[1:]):
        part = topk_exact(s[a:b], u[a:b], n_user, dom[a:b], n_domain, None if it is None else it[a:b], k + (a == 0))   # pass k >= k
        if acc is None:
            acc, acc_item = part, it
        else:
            acc = merge_exact(acc, part, n_user, n_domain, acc_item, None if it is None else it[a:b], k, row_offset=a)
    assert acc[0] == want[0]
    assert [[(r, float(v)) for r, v in l] for l in acc[2]] == [[(r, float(v)) for r, v in l] for l in want[2]]
    assert all(m <= w for m, w in zip(acc[1], want[1])) and any(m < w for m, w in zip(acc[1], want[1]))   # survivors: a lower bound
    # a k above a pass's cut is NOT served: the rows that pass dropped are gone
    short = topk_exact(s[:450], u[:450], n_user, dom[:450], n_domain, None if it is None else it[:450], 1)
    rest = topk_exact(s[450:], u[450:], n_user, dom[450:], n_domain, None if it is None else it[450:], k)
    merged = merge_exact(short, rest, n_user, n_domain, it, None if it is None else it[450:], k, row_offset=450)
    assert merged[0] == want[0] and merged[2] != want[2]


def test_cdc_eval_topk_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, 256-byte aligned, never dereferenced on the host
    big = 1 << 40

    def call(pred=p, user=p, n_user=100, domain=p, n_domain=3, item=p, k=10, n=10, n_out=p, gd=p, gu=p, gs=p, gr=p, er=p, es=p, ws=p,
             ws_bytes=big):
        return lib.cdc_eval_topk(pred, user, 1, n_user, domain, 1, n_domain, item, 1, k, n, n_out, gd, gu, gs, gr, er, es, None, ws,
                                 ws_bytes, None)

    for kw in ({"pred": None}, {"user": None}, {"n_out": None}, {"gd": None}, {"gu": None}, {"gs": None}, {"gr": None}, {"er": None},
               {"es": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.cdc_last_error(), kw
    for k in (0, -1):
        assert call(k=k) == -1 and b"at least one row" in lib.cdc_last_error(), k
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    assert call(n_user=(1 << 32) // 3 + 1) == -1 and b"exceed 2^32" in lib.cdc_last_error()
    assert call(n_user=(1 << 32) + 1, n_domain=1, domain=None) == -1 and b"exceed 2^32" in lib.cdc_last_error()
    assert call(n=1 << 31) == -1 and b"bad sizes" in lib.cdc_last_error()
    assert call(n=0) == -1 and call(n_user=0) == -1 and call(n_domain=0) == -1
    assert call(ws_bytes=64) == -1 and b"workspace 64 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    size = lib.cdc_eval_topk_workspace_bytes
    assert size(0, 3, 100, 0) == 0 and size(10, 4, (1 << 30) + 1, 1) == 0 and size(1 << 31, 1, 10, 0) == 0 and size(10, 0, 10, 0) == 0
    assert size(10, 4, 1 << 30, 1) != 0 and size(10, 1, 1 << 32, 0) != 0      # sizes the call serves (the byte count needs a device)


def test_eval_topk_host_mirror_checks_arguments():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import Evaluator, TopK, eval_topk
    pred, user = torch.rand(4), torch.zeros(4, dtype=torch.int32)
    for k in (0, -3, 2.5, 1 << 31, True):
        with pytest.raises(ValueError, match="k="):
            eval_topk(pred, user, n_user=10, k=k)
    with pytest.raises(ValueError, match="2\\^32"):
        eval_topk(pred, user, n_user=(1 << 31) + 1, domain=user, n_domain=2)
    with pytest.raises(ValueError, match="must be positive"):
        eval_topk(pred, user, n_user=0)
    with pytest.raises(_lib.HipExtensionError):
        eval_topk(pred, user, n_user=10)
    with pytest.raises(ValueError, match="user_idx"):
        Evaluator(None).recommend([])
    with pytest.raises(ValueError, match="by must be"):
        Evaluator(None, user_idx=1, n_user=4).recommend([], by="item")
    with pytest.raises(ValueError, match="domain_idx"):
        Evaluator(None, user_idx=1, n_user=4).recommend([])
    # dense / lists / merge on host tensors: plain torch
    t = TopK(torch.tensor([0, 1], dtype=torch.int32), torch.tensor([3, 0], dtype=torch.int32), torch.tensor([0, 2, 3], dtype=torch.int32),
             torch.tensor([4, 1], dtype=torch.int32), torch.tensor([7, 2, 5], dtype=torch.int32), torch.tensor([0.9, 0.1, 0.4]),
             torch.tensor([2, 3]), 3, 8, 4, 2)
    row, score = t.dense()
    assert row.tolist() == [[7, 2, -1], [5, -1, -1]] and row.dtype == torch.int32 and score.dtype == torch.float32
    assert score[0, :2].tolist() == t.score[:2].tolist() and torch.isnan(score).sum().item() == 3
    assert t.dense(fill=-9)[0][1].tolist() == [5, -9, -9]
    assert t.lists() == {(0, 3): ([7, 2], t.score[:2].tolist()), (1, 0): ([5], t.score[2:].tolist())}
    t.synced = False
    for call in (t.dense, t.lists, lambda: TopK.merge(t, t)):
        with pytest.raises(ValueError, match="sync=True"):
            call()
