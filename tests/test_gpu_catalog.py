"""cdc_catalog_rows / cdc_catalog_topk / CatalogTopK / Evaluator.recommend_catalog on the device against the plain-Python lists of
tests/catalog_exact.py.

No tolerance anywhere: the outputs are integers and bit-copied scores, and every field is compared for equality — item ids, catalogue
rows, score bits, the lists' lengths, the -1 / -1 / NaN (0x7fc00000) padding behind them and the error word.  Where the lists are
compared with Evaluator.recommend over the materialised pool, the forward sees the same batches on both routes, so the scores are
bit-equal and the comparison is for equality too."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from catalog_exact import HAND_ERR, HAND_IDS, HAND_K, HAND_LISTS, HAND_SCORE, HAND_SEEN, catalog_exact, dense, pool_rows

pytestmark = pytest.mark.gpu
FIELDS = ("item", "cat", "score", "n")


def _got(state):
    assert state.item.dtype == state.cat.dtype == state.n.dtype == torch.int32 and state.score.dtype == torch.float32
    out = {"item": state.item.cpu().numpy(), "cat": state.cat.cpu().numpy(), "score": state.score.cpu().numpy().view(np.uint32),
           "n": state.n.cpu().numpy(), "err": int(state.err.item())}
    return out


def _same(got, want, what=""):
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())
    assert got["err"] == want["err"], (what, got["err"], want["err"])


def _seen_dev(cuda, seen, U):
    from cdcmdr_amd.evaluate import catalog_seen
    if seen is None:
        return None
    ctx = [u for u, v in seen.items() for _ in v]
    item = [i for v in seen.values() for i in v]
    start, flat = catalog_seen(torch.tensor(ctx, dtype=torch.int64), torch.tensor(item, dtype=torch.int64), U)
    return start.to(cuda), flat.to(cuda)


def _catalog_dev(cuda, ids, n_cols=1):
    """the catalogue on the device: the id column alone, or column 0 of an [I, n_cols] matrix (a strided id column)"""
    cat = np.full((len(ids), n_cols), -9, dtype=np.int32)
    cat[:, 0] = ids
    return torch.from_numpy(cat).to(cuda)


def _fold(cuda, s, ids, k, seen=None, ub=None, ib=None, reverse=False, n_cols=1):
    """the pool's scores folded tile by tile into an empty state -> the state as numpy arrays"""
    from cdcmdr_amd.evaluate import CatalogTopK, catalog_topk
    s = np.asarray(s, dtype=np.float32)
    U, I = s.shape
    ub, ib = ub or U, ib or I
    score, cat, sn = torch.from_numpy(s).to(cuda), _catalog_dev(cuda, ids, n_cols), _seen_dev(cuda, seen, U)
    state = CatalogTopK.empty(U, k, cuda)
    i_tiles = list(range(0, I, ib))[::-1] if reverse else list(range(0, I, ib))
    for u0 in range(0, U, ub):
        for i0 in i_tiles:
            nu, ni = min(ub, U - u0), min(ib, I - i0)
            assert catalog_topk(state, score[u0:u0 + nu, i0:i0 + ni], cat, u0, nu, i0, ni, sn) is state
    assert catalog_topk.last_err is state.err
    return _got(state)


def _grid(rng, U, I, order="shuffled"):
    """scores on a 1/64 grid (heavy ties), every context's catalogue in the given score order"""
    s = (rng.integers(-64, 65, size=(U, I)) / 64).astype(np.float32)
    if order == "ascending":
        s = np.sort(s, axis=1)
    elif order == "descending":
        s = -np.sort(-s, axis=1)
    return s


def test_catalog_smallest_inputs(cuda):
    _same(_fold(cuda, [[0.25]], [5], 1), dense(catalog_exact([[0.25]], [5], 1), 1), "1x1x1")
    s, ids = [[0.5, -1.0, 0.5], [2.0, 2.0, 2.0]], [9, 4, 2]
    got = _fold(cuda, s, ids, 7)                                # k > I
    _same(got, dense(catalog_exact(s, ids, 7), 7), "k > I")
    assert got["n"].tolist() == [3, 3] and got["item"][0].tolist() == [2, 9, 4, -1, -1, -1, -1] and got["cat"][1].tolist()[:3] == [2, 1, 0]
    want = (HAND_LISTS, HAND_ERR)
    assert catalog_exact(HAND_SCORE, HAND_IDS, HAND_K, HAND_SEEN)[1] == HAND_ERR
    for n_cols in (1, 3):
        _same(_fold(cuda, HAND_SCORE, HAND_IDS, HAND_K, HAND_SEEN, n_cols=n_cols), dense(want, HAND_K), "hand example")
    _same(_fold(cuda, HAND_SCORE, HAND_IDS, HAND_K, HAND_SEEN, ub=1, ib=2, reverse=True), dense(want, HAND_K), "hand example, tiled")


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("k", [1, 10, 1024])
def test_catalog_refill_path(cuda, k, order):
    """I = 5000 > the 4096 entries of the buffer: ascending scores let every candidate beat the running threshold, so the buffer is
    compacted as often as it ever can be"""
    rng = np.random.default_rng(7 + k)
    U, I = 3, 5000
    s = _grid(rng, U, I, order)
    ids = rng.permutation(3 * I)[:I].astype(np.int32)
    _same(_fold(cuda, s, ids, k), dense(catalog_exact(s, ids, k), k), f"{order} k={k}")


def test_catalog_one_more_item_than_k_and_signed_zeros(cuda):
    rng = np.random.default_rng(3)
    s = _grid(rng, 2, 1025)
    ids = rng.permutation(5000)[:1025].astype(np.int32)
    got = _fold(cuda, s, ids, 1024)
    _same(got, dense(catalog_exact(s, ids, 1024), 1024), "I = 1025, k = 1024")
    assert got["n"].tolist() == [1024, 1024]
    # -0.0 against +0.0: one score, so the item id decides, and each entry keeps its own sign bit
    z = np.zeros((2, 40), dtype=np.float32)
    z[0, ::2] = -0.0
    z[1, 1::3] = -0.0
    z[1, 5] = 1.0
    zid = rng.permutation(100)[:40].astype(np.int32)
    got = _fold(cuda, z, zid, 12)
    _same(got, dense(catalog_exact(z, zid, 12), 12), "signed zeros")
    assert got["item"][0].tolist() == sorted(zid.tolist())[:12] and len(set(got["score"][0].tolist())) == 2
    # a misaligned score pointer with Ib a multiple of 4 takes the 4-byte loads
    from cdcmdr_amd.evaluate import CatalogTopK, catalog_topk
    buf = torch.zeros(1 + 2 * 1024, dtype=torch.float32, device=cuda)
    buf[1:].copy_(torch.from_numpy(s[:, :1024].reshape(-1)))
    assert buf[1:].data_ptr() % 16 == 4
    state = catalog_topk(CatalogTopK.empty(2, 5, cuda), buf[1:], _catalog_dev(cuda, ids[:1024]), 0, 2, 0, 1024)
    _same(_got(state), dense(catalog_exact(s[:, :1024], ids[:1024], 5), 5), "misaligned")


def _invariance_pool():
    rng = np.random.default_rng(21)
    U, I = 3, 2300
    s = _grid(rng, U, I)
    s[1, 17] = s[1, 2299] = np.nan
    ids = rng.permutation(3 * I)[:I].astype(np.int32)
    seen = {0: rng.choice(ids, size=200).tolist() + [10 ** 6], 2: rng.choice(ids, size=700).tolist()}
    return s, ids, seen


_INVARIANCE = {}


@pytest.mark.parametrize("ub", [1, 2, 3])
@pytest.mark.parametrize("k", [10, 1024])
def test_catalog_tile_invariance(cuda, k, ub):
    """every tile shape, item tiles folded forwards and backwards: the bits of the one-call result"""
    s, ids, seen = _invariance_pool()
    if k not in _INVARIANCE:                                    # the reference is computed once per k and left unchanged
        _INVARIANCE[k] = dense(catalog_exact(s, ids, k, seen), k)
        _same(_fold(cuda, s, ids, k, seen), _INVARIANCE[k], "one call")
    assert _INVARIANCE[k]["err"] == 2
    for ib in (1, 7, 1000, 2300):
        if ib == 1 and k == 1024 and ub != 3:
            continue                                            # 2300 launches per context row: once per k is enough at k = 1024
        for reverse in (False, True):
            _same(_fold(cuda, s, ids, k, seen, ub, ib, reverse), _INVARIANCE[k], f"ub={ub} ib={ib} reverse={reverse}")


def test_catalog_seen_sets(cuda):
    rng = np.random.default_rng(5)
    U, I, k = 5, 300, 8
    s = rng.random((U, I)).astype(np.float32)
    ids = (rng.permutation(I) * 3).astype(np.int32)             # multiples of 3: every other id is not in the catalogue
    top = [ids[np.argsort(-s[3], kind="stable")[:k]].tolist()]
    seen = {0: [],                                              # an empty slice
            1: [1, 2, 4, -5, 10 ** 6] + ids[:5].tolist() * 2,   # ids that are not in the catalogue, negative ones, duplicates
            2: ids.tolist(),                                    # everything seen
            3: top[0]}                                          # exactly the top k
    want = catalog_exact(s, ids, k, seen)
    assert want[0][2] == [] and not set(i for i, _, _ in want[0][3]) & set(top[0]) and len(want[0][3]) == k
    assert [i for i, _, _ in want[0][4]] == ids[np.argsort(-s[4], kind="stable")[:k]].tolist()
    for ib in (I, 64):
        got = _fold(cuda, s, ids, k, seen, ib=ib)
        _same(got, dense(want, k), f"seen ib={ib}")
        assert got["n"].tolist() == [k, k, 0, k, k] and (got["item"][2] == -1).all() and (got["score"][2] == 0x7fc00000).all()


def test_catalog_errors(cuda):
    rng = np.random.default_rng(6)
    U, I, k = 6, 200, 5
    s = rng.random((U, I)).astype(np.float32)
    ids = rng.permutation(1000)[:I].astype(np.int32)
    bad = s.copy()
    bad[1, 199] = bad[4, 0] = bad[4, 77] = np.nan               # a NaN score in two contexts
    bad[4, 78] = np.inf
    want = catalog_exact(bad, ids, k)
    assert want[1] == 5 and want[0][4][0][0] == ids[78]
    for ib in (I, 50):
        _same(_fold(cuda, bad, ids, k, ib=ib), dense(want, k), f"NaN ib={ib}")
    neg = ids.copy()
    neg[13] = -1
    s[:, 13] = 2.0                                              # the bad candidate would lead every list
    want = catalog_exact(s, neg, k)
    assert want[1] == U and all(13 not in [c for _, c, _ in l] for l in want[0])
    for ub, ib in ((U, I), (4, 50), (1, 13)):
        _same(_fold(cuda, s, neg, k, ub=ub, ib=ib), dense(want, k), f"negative id ub={ub} ib={ib}")
    # only the contexts of tiles that hold the negative id are flagged: the largest such context
    from cdcmdr_amd.evaluate import CatalogTopK, catalog_topk
    state = CatalogTopK.empty(U, k, cuda)
    catalog_topk(state, torch.from_numpy(s[1:4]).to(cuda), _catalog_dev(cuda, neg), 1, 3, 0, I)
    assert int(state.err.item()) == 4
    state = CatalogTopK.empty(U, k, cuda)
    catalog_topk(state, torch.from_numpy(s[:, 14:]).to(cuda), _catalog_dev(cuda, neg), 0, U, 14, I - 14)
    assert int(state.err.item()) == 0


def test_catalog_raw_call_writes_its_own_contexts_only(cuda):
    """caller-owned [U, k] buffers followed by a sentinel tail; a tile over contexts [1, 3) of 4"""
    from cdcmdr_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(8)
    U, I, k, tail = 4, 90, 6, 32
    s = rng.random((U, I)).astype(np.float32)
    ids = rng.permutation(500)[:I].astype(np.int32)
    item = torch.full((U * k + tail,), 77, dtype=torch.int32, device=cuda)
    cat = torch.full((U * k + tail,), 78, dtype=torch.int32, device=cuda)
    score = torch.full((U * k + tail,), 79.0, dtype=torch.float32, device=cuda)
    n = torch.full((U + tail,), 0, dtype=torch.int32, device=cuda)
    n[U:] = 80
    err = torch.zeros(1 + tail, dtype=torch.int32, device=cuda)
    tile = torch.from_numpy(s[1:3].copy()).to(cuda)
    catalog = _catalog_dev(cuda, ids, 2)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.cdc_catalog_topk(tile.data_ptr(), catalog.data_ptr(), 2, U, I, 1, 2, 0, I, None, None, 0, k, item.data_ptr(), cat.data_ptr(),
                              score.data_ptr(), n.data_ptr(), err.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    want = dense(catalog_exact(s[1:3], ids, k), k)
    item_h, cat_h, score_h, n_h = item.cpu().numpy(), cat.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(item_h[k:3 * k].reshape(2, k), want["item"]) and np.array_equal(cat_h[k:3 * k].reshape(2, k), want["cat"])
    assert np.array_equal(score_h[k:3 * k].view(np.uint32).reshape(2, k), want["score"]) and n_h[1:3].tolist() == want["n"].tolist()
    for lo, hi in ((0, k), (3 * k, U * k + tail)):              # contexts 0 and 3, and the tail
        assert (item_h[lo:hi] == 77).all() and (cat_h[lo:hi] == 78).all() and (score_h[lo:hi] == 79.0).all()
    assert n_h[0] == 0 and n_h[3] == 0 and (n_h[U:] == 80).all() and (err.cpu().numpy() == 0).all()


@pytest.mark.parametrize("F", [1, 5, 8, 26])
def test_catalog_rows_equal_the_torch_construction(cuda, F):
    from cdcmdr_amd.evaluate import catalog_rows
    rng = np.random.default_rng(F)
    U, I, n_domain = 7, 37, 4
    item_cols = [0] if F == 1 else [F - 1, 0]                   # the first and the last column
    domain_col = None if F == 1 else F // 2
    wide = torch.from_numpy(rng.integers(0, 1000, size=(U, F + 5)).astype(np.int32)).to(cuda)
    context = wide[:, 2:2 + F]                                  # a strided view
    assert context.stride(0) == F + 5
    if domain_col is not None:
        context[:, domain_col] = torch.from_numpy(rng.integers(0, n_domain, size=U).astype(np.int32)).to(cuda)
    catalog = torch.from_numpy(rng.integers(0, 1000, size=(I, len(item_cols))).astype(np.int32)).to(cuda)
    g_of_d = torch.tensor([2, 0, 1, 1], dtype=torch.int64, device=cuda)
    for u0, ub, i0, ib in ((0, U, 0, I), (2, 3, 5, 11), (6, 1, 36, 1), (0, 1, 0, I)):
        X, group, domain = catalog_rows(context, catalog, item_cols, u0, ub, i0, ib, None if domain_col is None else g_of_d, domain_col)
        want = torch.from_numpy(pool_rows(context.cpu().numpy(), catalog.cpu().numpy(), item_cols, u0, ub, i0, ib)).to(cuda)
        ref = context[u0:u0 + ub].repeat_interleave(ib, 0)
        for c, f in enumerate(item_cols):
            ref[:, f] = catalog[i0:i0 + ib, c].repeat(ub)
        assert X.dtype == torch.int32 and X.shape == (ub * ib, F) and torch.equal(X, ref) and torch.equal(X, want)
        if domain_col is None:
            assert group is None and domain is None
        else:
            assert domain.dtype == torch.int32 and domain.is_contiguous() and torch.equal(domain, ref[:, domain_col])
            assert group.dtype == torch.int64 and torch.equal(group, g_of_d[ref[:, domain_col].long()])
        assert int(catalog_rows.last_err.item()) == 0
    if domain_col is not None:                                  # an out-of-range domain: group 0, the word names the largest such context
        context[2, domain_col], context[5, domain_col] = n_domain, -1
        X, group, domain = catalog_rows(context, catalog, item_cols, 0, U, 0, I, g_of_d, domain_col)
        assert int(catalog_rows.last_err.item()) == 6 and domain[2 * I].item() == n_domain and domain[5 * I].item() == -1
        assert int(group[2 * I:3 * I].abs().sum().item()) == 0 and int(group[5 * I:6 * I].abs().sum().item()) == 0
        X, group, domain = catalog_rows(context, catalog, item_cols, 0, 5, 0, I, g_of_d, domain_col)
        assert int(catalog_rows.last_err.item()) == 3
        X, group, domain = catalog_rows(context, catalog, item_cols, 0, U, 0, I, None, domain_col)      # no table: nothing to flag
        assert group is None and int(catalog_rows.last_err.item()) == 0 and domain[2 * I].item() == n_domain


def _hash_scores(X, n_out, levels=1024):
    """an elementwise integer hash of every row of X mapped into (0, 1): [rows, n_out], column t hashed with t.  Row-independent, so
    tiling cannot change a bit; few levels, so scores tie"""
    h = torch.zeros(X.shape[0], dtype=torch.int64, device=X.device)
    for f in range(X.shape[1]):
        h = (h * 1000003 + X[:, f].to(torch.int64) + 12345) & 0xffffffff
    cols = []
    for t in range(n_out):
        g = ((h + 7919 * t) * 2654435761) & 0xffffffff
        g = ((g ^ (g >> 15)) * 2246822519) & 0xffffffff
        g = g ^ (g >> 13)
        cols.append((((g % levels).to(torch.float32) + 0.5) / levels))
    return torch.stack(cols, dim=1)


class _Stub(torch.nn.Module):
    def __init__(self, n_out):
        super().__init__()
        self.n_out = n_out

    def forward(self, X):
        return _hash_scores(X, self.n_out)


def test_catalog_replays_from_a_captured_graph(cuda):
    from cdcmdr_amd.evaluate import CatalogTopK, catalog_rows, catalog_topk
    rng = np.random.default_rng(9)
    U, I, F, k = 5, 700, 6, 9

    def draw():
        ctx = rng.integers(0, 50, size=(U, F)).astype(np.int32)
        cat = np.stack([rng.permutation(5000)[:I], rng.integers(0, 9, size=I)], axis=1).astype(np.int32)
        return ctx, cat
    first, second = draw(), draw()
    second[1][44, 0] = -3                                       # the error word is part of the replay
    context, catalog = torch.from_numpy(first[0]).to(cuda), torch.from_numpy(first[1]).to(cuda)
    state = CatalogTopK.empty(U, k, cuda)
    fresh = CatalogTopK.empty(U, k, cuda)

    def tile():
        X, _, _ = catalog_rows(context, catalog, [2, 4], 0, U, 0, I)
        catalog_topk(state, _hash_scores(X, 1), catalog, 0, U, 0, I)

    def reset():
        for f in FIELDS:
            getattr(state, f).copy_(getattr(fresh, f))
        state.err.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator
        tile()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tile()
    for data in (second, first):
        context.copy_(torch.from_numpy(data[0]))
        catalog.copy_(torch.from_numpy(data[1]))
        reset()
        graph.replay()
        torch.cuda.synchronize()
        replayed = _got(state)
        reset()
        tile()                                                  # eager
        _same(replayed, _got(state), "graph against eager")
        s = _hash_scores(torch.from_numpy(pool_rows(data[0], data[1], [2, 4])).to(cuda), 1).reshape(U, I).cpu().numpy()
        _same(replayed, dense(catalog_exact(s, data[1][:, 0], k), k), "graph against the restatement")
    assert replayed["err"] == 0


def _recommend_lists(top):
    """a synced TopK with items -> {(domain, user): [(item, score bits)]}"""
    dom, usr, start = top.domain.cpu().tolist(), top.user.cpu().tolist(), top.start.cpu().tolist()
    item, score = top.item.cpu().tolist(), top.score.cpu().numpy().view(np.uint32).tolist()
    return {(dom[j], usr[j]): list(zip(item[start[j]:start[j + 1]], score[start[j]:start[j + 1]])) for j in range(len(dom))}


def _catalog_lists(state, context, domain_col, user_col):
    got = _got(state)
    ctx = context.cpu().numpy()
    return {(int(ctx[u, domain_col]), int(ctx[u, user_col])): list(zip(got["item"][u, :got["n"][u]].tolist(), got["score"][u, :got["n"][u]].tolist()))
            for u in range(ctx.shape[0])}


def _pool_loader(cuda, context, catalog, item_cols, bs, g_of_d=None, domain_col=None):
    X = torch.from_numpy(pool_rows(context.cpu().numpy(), catalog.cpu().numpy(), item_cols)).to(cuda)
    y = torch.zeros((X.shape[0], 1), dtype=torch.int16, device=cuda)
    y[::3] = 1
    if g_of_d is None:
        return X, [(X[i:i + bs], y[i:i + bs]) for i in range(0, X.shape[0], bs)]
    g = torch.as_tensor(g_of_d, dtype=torch.int64, device=cuda)[X[:, domain_col].long()].reshape(-1, 1)
    return X, [(X[i:i + bs], y[i:i + bs], g[i:i + bs]) for i in range(0, X.shape[0], bs)]


@pytest.mark.parametrize("mode", ["single", "multi"])
def test_recommend_catalog_with_a_stub_model(cuda, mode):
    from cdcmdr_amd.evaluate import Evaluator
    rng = np.random.default_rng(10)
    U, I, F, k, n_domain, n_user = 11, 130, 6, 7, 3, 40         # columns: 1 item, 2 item side feature, 3 user, 4 domain
    ctx = rng.integers(0, 30, size=(U, F)).astype(np.int32)
    ctx[:, 3] = rng.permutation(n_user)[:U]                     # distinct users: distinct (domain, user)
    ctx[:, 4] = rng.integers(0, n_domain, size=U)
    cat = np.stack([rng.permutation(900)[:I], rng.integers(0, 5, size=I)], axis=1).astype(np.int32)
    context, catalog, item_cols = torch.from_numpy(ctx).to(cuda), torch.from_numpy(cat).to(cuda), [1, 2]
    d2g = [1, 0, 1]
    model = _Stub(2 if mode == "multi" else 1).to(cuda)
    ev = Evaluator(model, mode=mode, domain_idx=4, n_domain=n_domain, user_idx=3, n_user=n_user)
    X, loader = _pool_loader(cuda, context, catalog, item_cols, 500, d2g if mode == "multi" else None, 4)
    out = model(X)
    s = (out.gather(1, torch.tensor(d2g, device=cuda)[X[:, 4].long()].reshape(-1, 1)) if mode == "multi" else out).reshape(U, I).cpu().numpy()
    seen = {u: rng.choice(cat[:, 0], size=20).tolist() for u in range(0, U, 3)}
    for sn in (None, seen):
        want = dense(catalog_exact(s, cat[:, 0], k, sn), k)
        for tile_rows, item_block in ((64, None), (1000, None), (U * I, None), (300, 50)):
            state = ev.recommend_catalog(context, catalog, item_cols, k=k, seen=_seen_dev(cuda, sn, U), domain2group=d2g if mode == "multi" else None,
                                         tile_rows=tile_rows, item_block=item_block)
            _same(_got(state), want, f"{mode} tile_rows={tile_rows} seen={sn is not None}")
            assert state.k == k and state.lists()[0][0] == want["item"][0, :want["n"][0]].tolist()
    # read as (item, score) lists: Evaluator.recommend over the materialised pool
    state = ev.recommend_catalog(context, catalog, item_cols, k=k, domain2group=d2g if mode == "multi" else None, tile_rows=64)
    top = ev.recommend(loader, k=k, item_idx=1, by="domain")
    assert _catalog_lists(state, context, 4, 3) == _recommend_lists(top)
    if mode == "multi":
        bad = context.clone()
        bad[6, 4] = n_domain
        with pytest.raises(ValueError, match="context 6: domain outside"):
            ev.recommend_catalog(bad, catalog, item_cols, k=k, domain2group=d2g, tile_rows=64)
    neg = catalog.clone()
    neg[:, 0] = neg[:, 0] - 2000                                # the up-front check
    with pytest.raises(ValueError, match="negative item id"):
        ev.recommend_catalog(context, neg, item_cols, k=k, domain2group=d2g)


class _NaNAt(torch.nn.Module):
    """the stub with a NaN wherever column 1 (the item) holds `item`"""

    def __init__(self, item):
        super().__init__()
        self.item = item

    def forward(self, X):
        out = _hash_scores(X, 1)
        out[X[:, 1] == self.item] = float("nan")
        return out


def test_recommend_catalog_raises_for_a_nan_prediction(cuda):
    from cdcmdr_amd.evaluate import Evaluator
    context = torch.arange(24, dtype=torch.int32, device=cuda).reshape(4, 6)
    catalog = torch.arange(10, dtype=torch.int32, device=cuda).reshape(10, 1) * 7
    with pytest.raises(ValueError, match="context 3: NaN prediction"):
        Evaluator(_NaNAt(21), mode="single").recommend_catalog(context, catalog, [1], k=3, tile_rows=8)


def _cdc_config():
    return types.SimpleNamespace(mmoe_n_expert=4, ple_n_expert_specific=2, ple_n_expert_shared=2, gate_hidden_dim=8, dataset_name="t",
                                 p_weight=0.5, p_weight_method="none", old_matrix_weight=0.0, affinity_func="minus", use_atten=False,
                                 n_cross_layers=3)


def test_recommend_catalog_with_a_real_ple_and_a_cdc_ple(cuda):
    """every tile is 4 whole contexts x all 64 items and the loader's batches are those tiles, so both routes score identical batches"""
    from cdcmdr_amd.evaluate import Evaluator
    from cdcmdr_amd.model.cdc import CDC
    from cdcmdr_amd.model.ple import PLE
    FD = [30, 2000, 7, 300, 3]                                  # column 1: 2000 items, column 3: 300 users, column 4: 3 domains
    rng = np.random.default_rng(12)
    U, I, k, ub = 12, 64, 5, 4
    ctx = np.stack([rng.integers(0, d, size=U) for d in FD], axis=1).astype(np.int32)
    ctx[:, 3] = rng.permutation(300)[:U]
    cat = np.stack([rng.permutation(2000)[:I], rng.integers(0, 7, size=I)], axis=1).astype(np.int32)
    context, catalog, item_cols = torch.from_numpy(ctx).to(cuda), torch.from_numpy(cat).to(cuda), [1, 2]
    d2g = [0, 1, 2]
    torch.manual_seed(3)
    ple = PLE(FD, 8, 3, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.2).to(cuda).set_precision("f32")
    kw = dict(mode="multi", domain_idx=4, n_domain=3, user_idx=3, n_user=300)
    X, loader = _pool_loader(cuda, context, catalog, item_cols, ub * I, d2g, 4)
    ev = Evaluator(ple, **kw)
    recal = ev.fit_recalibration(loader)                        # isotonic: plateaus make ties, which fall back to the item id
    for e in (ev, Evaluator(ple, recalibration=recal, **kw)):
        state = e.recommend_catalog(context, catalog, item_cols, k=k, domain2group=d2g, tile_rows=ub * I)
        top = e.recommend(loader, k=k, item_idx=1, by="domain")
        got = _catalog_lists(state, context, 4, 3)
        assert got == _recommend_lists(top) and all(len(l) == k for l in got.values())
        pred = e.predict(loader)[0].reshape(U, I).cpu().numpy()
        _same(_got(state), dense(catalog_exact(pred, cat[:, 0], k), k), "ple")
    assert ple.training
    tied = Evaluator(ple, recalibration=recal, **kw).predict(loader)[0].reshape(U, I).cpu().numpy()
    assert any(len(set(row.tolist())) < I for row in tied)      # the recalibrated scores do tie
    # CDC around a PLE: split mode gathers by the model's own domain2group
    torch.manual_seed(4)
    cdc = CDC(FD, 8, 2, 3, "ple", ((32, 16), (8,)), (8, 4), 4, n_causal_mask=2, device=cuda, dropout=0.2, config=_cdc_config())
    cdc = cdc.to(cuda).set_precision("f32")
    cdc.domain2group.copy_(torch.tensor([1, 0, 1]))
    cdc.domain2group_list = [1, 0, 1]
    state = Evaluator(cdc, mode="cdc", domain_idx=4, n_domain=3).recommend_catalog(context, catalog, item_cols, k=k, tile_rows=ub * I)
    cdc.eval()
    with torch.no_grad():
        pred = torch.cat([cdc(X[i:i + ub * I], mode="split").reshape(-1) for i in range(0, U * I, ub * I)]).reshape(U, I).cpu().numpy()
    cdc.train()
    _same(_got(state), dense(catalog_exact(pred, cat[:, 0], k), k), "cdc")
