"""cdc_eval_topk / eval_topk / TopK / Evaluator.recommend on the device against the plain-Python lists of tests/topk_exact.py.

No tolerance anywhere: the outputs are integers and bit-copied scores, and every field is compared for equality — the groups, the
starts with start[G] == E, the survivor counts before the cut, the rows, the score bits, the gathered items and the error word.  The
one derived bound is in the cross-check against eval_rank, whose figures are floating-point: (2 K + 2 G + 8) 2^-53, the bound of
tests/test_gpu_rank.py for that call."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from topk_exact import flat, topk_exact

pytestmark = pytest.mark.gpu
K_ALL = 2 ** 31 - 1
FIELDS = ("domain", "user", "start", "rows", "row", "score")


def _columns(cuda, u, dom, item, strided):
    """the id columns on the device: contiguous, or views of one [n, 5] id matrix"""
    n = len(u)
    if strided:
        X = np.full((n, 5), -7, dtype=np.int32)
        X[:, 3] = u
        X[:, 0] = dom if dom is not None else 0
        X[:, 4] = item if item is not None else 0
        Xd = torch.from_numpy(X).to(cuda)
        cols = Xd[:, 3], (Xd[:, 0] if dom is not None else None), (Xd[:, 4] if item is not None else None)
        assert cols[0].stride(0) == 5
        return cols
    as_dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a).astype(np.int32)).to(cuda)
    return as_dev(u), as_dev(dom), as_dev(item)


def _got(t, err):
    """a synced TopK -> the dict of tests/topk_exact.flat"""
    G, E = t.n_out.cpu().tolist()
    assert t.domain.numel() == t.user.numel() == t.rows.numel() == G and t.start.numel() == G + 1
    assert t.row.numel() == t.score.numel() == E
    for f in FIELDS[:5]:
        assert getattr(t, f).dtype == torch.int32 and getattr(t, f).is_cuda
    assert t.score.dtype == torch.float32
    out = {f: getattr(t, f).cpu().numpy() for f in FIELDS[:5]}
    out["score"] = t.score.cpu().numpy().view(np.uint32)
    out["err"] = err
    return out


def _device(cuda, s, u, n_user, dom=None, n_domain=1, item=None, k=10, strided=False):
    from cdcmdr_amd.evaluate import eval_topk
    pred = torch.from_numpy(np.asarray(s, dtype=np.float32)).to(cuda)
    ut, dt, it = _columns(cuda, u, dom, item, strided)
    t = eval_topk(pred, ut, n_user, dt, n_domain, it, k)
    assert t.err is eval_topk.last_err and t.k == k and t.synced
    got = _got(t, int(t.err.item()))
    if item is not None:
        assert t.item.dtype == torch.int32
        assert t.item.cpu().numpy().tolist() == np.asarray(item)[got["row"]].tolist()
    else:
        assert t.item is None
    return got


def _same(got, want, what=""):
    G = len(want["domain"])
    assert len(got["start"]) == G + 1 and got["start"][G] == len(want["row"]), what           # start[G] == E
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].tolist() == want[f].tolist(), (what, f)
    assert got["err"] == want["err"], (what, got["err"], want["err"])


def _cut(full, k):
    """the helper's full rankings cut at k (tests/test_topk_cpu.py pins that the helper's cut is this)"""
    return full[0], full[1], [l[:k] for l in full[2]], full[3]


def test_topk_smallest_inputs(cuda):
    for k in (1, 7, K_ALL):
        _same(_device(cuda, [0.25], [0], 1, k=k), flat(topk_exact([0.25], [0], 1, k=k)), f"n=1 k={k}")
        _same(_device(cuda, [0.25], [2], 3, [1], 2, [9], k=k), flat(topk_exact([0.25], [2], 3, [1], 2, [9], k=k)), f"n=1 item k={k}")
    s, u, dom, item = [0.5, 0.9, 0.9, 0.1, -0.0, 0.0, 0.3, 0.9, 0.0], [1, 1, 1, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 1, 0, 0, 1], [5, 5, 7, 3, 2, 1, 9, 7, 2]
    got = _device(cuda, s, u, 2, dom, 2, item, 2)               # the hand example of tests/test_topk_cpu.py
    assert got["row"].tolist() == [6, 1, 2, 5, 4] and got["rows"].tolist() == [1, 3, 2] and got["start"].tolist() == [0, 1, 3, 5]
    for it in (None, item):
        for d, nd in ((dom, 2), (None, 1)):
            for k in (1, 2, K_ALL):
                _same(_device(cuda, s, u, 2, d, nd, it, k), flat(topk_exact(s, u, 2, d, nd, it, k)), f"hand {it is None} {nd} {k}")


@functools.lru_cache(maxsize=None)
def _big():
    """70 001 rows over 3 domains: (domain 1, user 7) owns 40 000 of them — a group across many sort and scan blocks — and the rest are
    Zipf-spread over 5 000 users; scores on a 1/1000 grid (long tie runs), items from 3 000 ids.  Full rankings, computed once."""
    n, n_user, n_domain = 70001, 5000, 3
    rng = np.random.default_rng(70001)
    u = np.minimum(rng.zipf(1.3, size=n) - 1, n_user - 1).astype(np.int64)
    dom = rng.integers(0, n_domain, size=n)
    own = rng.permutation(n)[:40000]
    u[own], dom[own] = 7, 1
    s = np.round(rng.random(n), 3).astype(np.float32)
    item = rng.integers(0, 3000, size=n)
    plain = topk_exact(s, u, n_user, dom, n_domain, None, K_ALL)
    dedup = topk_exact(s, u, n_user, dom, n_domain, item, K_ALL)
    assert plain[1][plain[0].index((1, 7))] >= 40000 and 1024 < dedup[1][dedup[0].index((1, 7))] <= 3000
    return s, u, dom, item, n_user, n_domain, plain, dedup


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_topk_group_across_sort_and_scan_blocks(cuda, k):
    s, u, dom, item, n_user, n_domain, plain, dedup = _big()
    _same(_device(cuda, s, u, n_user, dom, n_domain, None, k), flat(_cut(plain, k)), f"big k={k}")
    _same(_device(cuda, s, u, n_user, dom, n_domain, item, k), flat(_cut(dedup, k)), f"big item k={k}")


def _heavy_ties(n, n_user, n_domain, seed):
    rng = np.random.default_rng(seed)
    s = rng.choice(np.array([0.0, -0.0, 0.125, 0.25, 0.5, 0.75, 1.0, -1.0], dtype=np.float32), size=n)   # 8 values, 7 distinct scores
    s[rng.integers(0, n, size=n // 8)] = np.float32(3.5)                                                # ... 8 with this one
    return s, rng.integers(0, n_user, size=n), rng.integers(0, n_domain, size=n), rng.integers(0, 12, size=n)


@pytest.mark.parametrize("with_item", [False, True])
def test_topk_heavy_ties(cuda, with_item):
    n, n_user, n_domain = 6000, 37, 3
    s, u, dom, item = _heavy_ties(n, n_user, n_domain, 21)
    assert len(set((s + np.float32(0.0)).tolist())) == 8 and (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any()
    it = item if with_item else None
    full = topk_exact(s, u, n_user, dom, n_domain, it, K_ALL)
    for k in (1, 5, 12, K_ALL):
        _same(_device(cuda, s, u, n_user, dom, n_domain, it, k), flat(_cut(full, k)), f"ties k={k}")
    by_user = topk_exact(s, u, n_user, None, 1, it, 5)
    _same(_device(cuda, s, u, n_user, None, 1, it, 5), flat(by_user), "ties by user")
    if with_item:
        assert max(full[1]) <= 12 and sum(full[1]) < n // 4     # duplicates abound


def _raw(cuda, s, u, n_user, dom, n_domain, item, k, n_user_arg=None, n_domain_arg=None, short=0, tail=64):
    """cdc_eval_topk through ctypes with caller-owned outputs of capacity n (start: n + 1) followed by a sentinel-filled tail
    -> (rc, outputs by name, n)"""
    from cdcmdr_amd import _lib
    lib = _lib.load()
    n = len(s)
    pred = torch.from_numpy(np.asarray(s, dtype=np.float32)).to(cuda)
    ut, dt, it = _columns(cuda, u, dom, item, False)
    SENT = 0x5A5A5A5A
    bufs = {"n_out": torch.full((2 + tail,), SENT, dtype=torch.int64, device=cuda)}
    for name in ("domain", "user", "start", "rows", "row", "score_bits"):
        bufs[name] = torch.full((n + (name == "start") + tail,), SENT, dtype=torch.int32, device=cuda)
    err = torch.zeros(1 + tail, dtype=torch.int32, device=cuda)
    nbytes = lib.cdc_eval_topk_workspace_bytes(n, n_domain, n_user, int(item is not None))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    assert ws.data_ptr() % 256 == 0
    rc = lib.cdc_eval_topk(pred.data_ptr(), ut.data_ptr(), 1, n_user if n_user_arg is None else n_user_arg,
                           None if dt is None else dt.data_ptr(), 1, n_domain if n_domain_arg is None else n_domain_arg,
                           None if it is None else it.data_ptr(), 1, k, n, bufs["n_out"].data_ptr(), bufs["domain"].data_ptr(),
                           bufs["user"].data_ptr(), bufs["start"].data_ptr(), bufs["rows"].data_ptr(), bufs["row"].data_ptr(),
                           bufs["score_bits"].data_ptr(), err.data_ptr(), ws.data_ptr(), nbytes - short,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    bufs["err"] = err
    return rc, {name: b.cpu().numpy() for name, b in bufs.items()}, n


def _untouched(out, n, from_start=False):
    SENT = 0x5A5A5A5A
    for name, a in out.items():
        if name == "err":
            assert (a == 0).all() if from_start else (a[1:] == 0).all()
            continue
        cap = 0 if from_start else (2 if name == "n_out" else n + (name == "start"))
        assert (a[cap:] == SENT).all(), name


def test_topk_group_ids_at_the_top_of_the_key(cuda):
    n, n_domain, n_user = 4096, 4, 1 << 30                      # n_domain * n_user == 2^32 exactly: group ids up to 2^32 - 1
    rng = np.random.default_rng(4096)
    pool = np.concatenate([[0, 1, n_user - 2, n_user - 1], rng.integers(0, n_user, size=200)]).astype(np.int64)
    u = pool[rng.integers(0, len(pool), size=n)]
    u[:8] = [0, 1, n_user - 2, n_user - 1, 0, 1, n_user - 2, n_user - 1]
    dom = rng.integers(0, n_domain, size=n)
    dom[:8] = [0, 0, 0, 0, 3, 3, 3, 3]
    s = np.round(rng.random(n), 2).astype(np.float32)
    s[3], s[7] = -np.inf, -np.inf                               # the key closest to the excluded rows' all-ones key: group 2^32 - 1, -inf
    s[9] = np.nan
    item = rng.integers(0, 2 ** 31 - 1, size=n)
    item[:4] = [0, 2 ** 31 - 1, 0, 2 ** 31 - 1]
    for it in (None, item):
        for k in (3, K_ALL):
            want = topk_exact(s, u, n_user, dom, n_domain, it, k)
            assert want[0][0] == (0, 0) and want[0][-1] == (3, n_user - 1) and want[3] == 10
            _same(_device(cuda, s, u, n_user, dom, n_domain, it, k, strided=True), flat(want), f"top ids k={k}")
    # n_domain * n_user = 2^32 + 1 (and the next products a column pair can have): refused before anything is launched or written
    for nd, nu in ((1, (1 << 32) + 1), (4, (1 << 30) + 1), (3, (1 << 32) // 3 + 1)):
        rc, out, _ = _raw(cuda, s[:64], np.zeros(64), 5, dom[:64] % nd, nd, None, 3, n_user_arg=nu)
        assert rc == -1, (nd, nu)
        _untouched(out, 64, from_start=True)


def test_topk_excluded_rows(cuda):
    rng = np.random.default_rng(31)
    n, n_user, n_domain = 3000, 50, 3
    s = np.round(rng.random(n), 2).astype(np.float32)
    u, dom, item = rng.integers(0, n_user, size=n), rng.integers(0, n_domain, size=n), rng.integers(0, 40, size=n)
    _same(_device(cuda, s, u, n_user, dom, n_domain, item, 5), flat(topk_exact(s, u, n_user, dom, n_domain, item, 5)), "clean")
    cases = []
    for where, what in ((1234, "nan"), (2999, "user_max"), (0, "user_neg"), (77, "user_n"), (1500, "dom_neg"), (2998, "dom_n"), (600, "item_neg")):
        s2, u2, d2, i2 = s.copy(), u.copy(), dom.copy(), item.copy()
        if what == "nan":
            s2[where] = np.nan
        elif what.startswith("user"):
            u2[where] = {"user_max": 2 ** 31 - 1, "user_neg": -1, "user_n": n_user}[what]
        elif what.startswith("dom"):
            d2[where] = {"dom_neg": -1, "dom_n": n_domain}[what]
        else:
            i2[where] = -5
        cases.append((what, where, s2, u2, d2, i2))
    for what, where, s2, u2, d2, i2 in cases:
        for it in (i2, None):
            want = topk_exact(s2, u2, n_user, d2, n_domain, it, 5)
            assert want[3] == (0 if what == "item_neg" and it is None else where + 1)
            got = _device(cuda, s2, u2, n_user, d2, n_domain, it, 5)
            _same(got, flat(want), what)
            if want[3]:
                assert where not in got["row"].tolist()
    # all four at once, k above every group: the rows are absent from every list and the word is the largest index
    s2, u2, d2, i2 = s.copy(), u.copy(), dom.copy(), item.copy()
    s2[10], u2[20], d2[30], i2[40] = np.nan, 2 ** 31 - 1, -1, -5
    want = topk_exact(s2, u2, n_user, d2, n_domain, i2, K_ALL)
    got = _device(cuda, s2, u2, n_user, d2, n_domain, i2, K_ALL)
    _same(got, flat(want), "four")
    assert want[3] == 41 and not {10, 20, 30, 40} & set(got["row"].tolist())
    # nothing survives: G = E = 0 and start[0] = 0
    got = _device(cuda, np.full(5, np.nan, dtype=np.float32), [0] * 5, 2, k=3)
    _same(got, flat(topk_exact(np.full(5, np.nan, dtype=np.float32), [0] * 5, 2, k=3)), "none")
    assert got["start"].tolist() == [0] and got["err"] == 5


def test_topk_writes_nothing_past_the_capacity(cuda):
    rng = np.random.default_rng(41)
    n, n_user = 5000, 5000
    s = rng.random(n).astype(np.float32)
    for u, item, what in ((np.arange(n), None, "every row its own group: G = E = n"), (np.zeros(n), None, "one group, full ranking: E = n"),
                          (rng.integers(0, 300, size=n), rng.integers(0, 50, size=n), "items")):
        rc, out, _ = _raw(cuda, s, u, n_user, None, 1, item, K_ALL)
        assert rc == 0, what
        _untouched(out, n)
        want = flat(topk_exact(s, u, n_user, None, 1, item, K_ALL))
        G, E = out["n_out"][:2].tolist()
        assert (G, E) == (len(want["domain"]), len(want["row"])), what
        got = {"domain": out["domain"][:G], "user": out["user"][:G], "start": out["start"][:G + 1], "rows": out["rows"][:G],
               "row": out["row"][:E], "score": out["score_bits"][:E].view(np.uint32), "err": int(out["err"][0])}
        _same(got, want, what)
    rc, out, _ = _raw(cuda, s, np.zeros(n), n_user, None, 1, None, 3, short=1)
    assert rc == -1                                             # a workspace one byte short
    _untouched(out, n, from_start=True)


def test_topk_workspace_is_linear_in_the_rows_alone(cuda):
    from cdcmdr_amd import _lib
    size = _lib.load().cdc_eval_topk_workspace_bytes
    assert size(5000, 1, 10, 0) == size(5000, 4, 1 << 30, 0) > 0 and size(5000, 3, 100, 0) % 256 == 0
    assert size(5000, 3, 100, 1) >= size(5000, 3, 100, 0)
    assert size(1 << 24, 3, 100, 1) < 64 * (1 << 24)            # a few words per row


def test_topk_item_lists_do_not_depend_on_the_row_order(cuda):
    n, n_user, n_domain = 6000, 37, 3
    s, u, dom, item = _heavy_ties(n, n_user, n_domain, 51)
    rng = np.random.default_rng(52)

    def sequences(p):
        got = _device(cuda, s[p], u[p], n_user, dom[p], n_domain, item[p], 5)
        it = item[p][got["row"]]
        sc = got["score"].view(np.float32) + np.float32(0.0)
        return got["domain"].tolist(), got["user"].tolist(), got["start"].tolist(), got["rows"].tolist(), it.tolist(), sc.tolist()
    first = sequences(np.arange(n))
    for _ in range(2):
        assert sequences(rng.permutation(n)) == first
    a, b = _device(cuda, s, u, n_user, dom, n_domain, item, 5), _device(cuda, s, u, n_user, dom, n_domain, item, 5)
    _same(a, b, "same input, same bits")


def test_topk_replays_from_a_captured_graph(cuda):
    from cdcmdr_amd.evaluate import eval_topk
    n, n_user, n_domain, k = 3000, 200, 3, 4
    rng = np.random.default_rng(9)

    def draw():
        return (np.round(rng.random(n), 2).astype(np.float32), rng.integers(0, n_user, size=n).astype(np.int32),
                rng.integers(0, n_domain, size=n).astype(np.int32), rng.integers(0, 30, size=n).astype(np.int32))
    first, second = draw(), draw()
    second[0][5], second[1][17] = np.nan, n_user                # the error word is part of the replay
    bufs = [torch.from_numpy(a).to(cuda) for a in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator
        eval_topk(bufs[0], bufs[1], n_user, bufs[2], n_domain, bufs[3], k, sync=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t = eval_topk(bufs[0], bufs[1], n_user, bufs[2], n_domain, bufs[3], k, sync=False)
        err = eval_topk.last_err
    assert not t.synced and t.row.numel() == n and t.start.numel() == n + 1 and t.item.numel() == n
    with pytest.raises(ValueError, match="sync=True"):
        t.lists()
    for data in (second, first):
        for b, a in zip(bufs, data):
            b.copy_(torch.from_numpy(a))
        graph.replay()                                          # eval_topk zeroes the error word inside the capture
        torch.cuda.synchronize()
        s, u, dom, item = data
        want = flat(topk_exact(s, u, n_user, dom, n_domain, item, k))
        G, E = t.n_out.cpu().tolist()
        assert (G, E) == (len(want["domain"]), len(want["row"]))
        got = {"domain": t.domain[:G], "user": t.user[:G], "start": t.start[:G + 1], "rows": t.rows[:G], "row": t.row[:E]}
        got = {f: v.cpu().numpy() for f, v in got.items()}
        got["score"] = t.score[:E].cpu().numpy().view(np.uint32)
        got["err"] = int(err.item())
        _same(got, want, "graph")
        assert t.item[:E].cpu().numpy().tolist() == item[got["row"]].tolist()


def test_topk_lists_reproduce_eval_rank(cuda):
    """precision, recall and hit rate recomputed on the host from the device lists and the labels against eval_rank's device values:
    tie-free scores, so the expectation over tie orders is the one order the lists hold.  Bound: that call's (2 K + 2 G + 8) 2^-53."""
    from cdcmdr_amd.evaluate import eval_rank
    n, n_user, n_domain, ks = 20000, 700, 3, (1, 5, 10)
    rng = np.random.default_rng(61)
    s = (rng.permutation(n) / n).astype(np.float32)
    assert len(set(s.tolist())) == n
    y, u, dom = rng.integers(0, 2, size=n), rng.integers(0, n_user, size=n), rng.integers(0, n_domain, size=n)
    pred, label = torch.from_numpy(s).to(cuda), torch.from_numpy(y.astype(np.int16)).to(cuda)
    ut, dt, _ = _columns(cuda, u, dom, None, False)
    r = eval_rank(pred, label, ut, n_user, dt, n_domain, ks)
    figs = {f: getattr(r, f).cpu().numpy() for f in ("precision", "recall", "hit")}
    counted = r.counted.cpu().tolist()
    P_dom = np.zeros((n_domain, n_user), dtype=np.int64)
    np.add.at(P_dom, (dom, u), y)
    for d_col, nd in ((dom, n_domain), (None, 1)):              # the per-domain call serves segments 0..n_domain-1, the other ALL
        got = _device(cuda, s, u, n_user, d_col, nd, None, ks[-1])
        segs = range(n_domain) if d_col is not None else [n_domain]
        for sg in segs:
            P = P_dom[sg] if d_col is not None else P_dom.sum(axis=0)
            sums, G = {K: [Fraction(0)] * 3 for K in ks}, 0
            for j in range(len(got["user"])):
                if d_col is not None and got["domain"][j] != sg:
                    continue
                Pg = int(P[got["user"][j]])
                if Pg == 0:
                    continue
                G += 1
                rows = got["row"][got["start"][j]:got["start"][j + 1]]
                for K in ks:
                    hits = int(y[rows[:K]].sum())
                    sums[K] = [sums[K][0] + Fraction(hits, K), sums[K][1] + Fraction(hits, Pg), sums[K][2] + (1 if hits else 0)]
            assert G == counted[sg] and G > 100
            for q, K in enumerate(ks):
                for f, v in zip(("precision", "recall", "hit"), sums[K]):
                    diff = abs(Fraction(float(figs[f][q, sg])) - v / G)
                    assert diff <= (2 * K + 2 * G + 8) * Fraction(1, 2 ** 53), (sg, f, K, float(diff * 2 ** 53))


def _equal_topk(a, b, what=""):
    for f in FIELDS + ("item", "label"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (what, f)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
            assert (x.view(torch.int32) == y.view(torch.int32)).all() if x.dtype == torch.float32 else (x == y).all(), (what, f)


def test_evaluator_recommend_in_multi_and_single_mode(cuda):
    from cdcmdr_amd.evaluate import Evaluator, eval_topk
    from cdcmdr_amd.model.dcn import DCN
    from cdcmdr_amd.model.ple import PLE
    FD = [30, 2000, 7, 300, 3]                                  # column 1: 2000 items, column 3: 300 users, column 4: 3 domains
    torch.manual_seed(3)
    ple = PLE(FD, 8, 3, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.2).to(cuda).set_precision("f32")
    torch.manual_seed(4)
    dcn = DCN(FD, 8, 2, (16, 8), dropout=0.0).to(cuda).set_precision("f32")
    rng = np.random.default_rng(5)
    n, bs = 2500, 1024                                          # ragged last batch
    X = np.stack([rng.integers(0, d, size=n) for d in FD], axis=1).astype(np.int32)
    X[:, 1] = rng.integers(0, 60, size=n)                       # few items: a user meets one twice
    y = rng.integers(0, 2, size=n).astype(np.int16)
    g = X[:, 4].astype(np.int64)
    loader = [(torch.from_numpy(X[i:i + bs]).to(cuda), torch.from_numpy(y[i:i + bs]).to(cuda).reshape(-1, 1),
               torch.from_numpy(g[i:i + bs]).to(cuda).reshape(-1, 1)) for i in range(0, n, bs)]
    Xd = torch.from_numpy(X).to(cuda)
    for model, mode, data in ((ple, "multi", loader), (dcn, "single", [(a, b) for a, b, _ in loader])):
        kw = dict(mode=mode, domain_idx=4, n_domain=3, domain_cnt_weight={0: 0.5, 1: 0.3, 2: 0.2}, user_idx=3, n_user=300)
        ev = Evaluator(model, **kw)
        before = ev.test(data)
        pred, label, dom = ev.predict(data)
        for by in ("domain", "user"):
            for item_idx in (None, 1):
                top = ev.recommend(data, k=5, item_idx=item_idx, by=by)
                item = None if item_idx is None else Xd[:, item_idx]
                want = eval_topk(pred, Xd[:, 3], 300, dom if by == "domain" else None, 3 if by == "domain" else 1, item, 5)
                want.label = label[want.row.to(torch.int64)]
                _equal_topk(top, want, f"{mode} {by} {item_idx}")
                assert top.label.dtype == torch.int16 and top.k == 5 and top.n == n
                assert top.label.cpu().numpy().tolist() == y[top.row.cpu().numpy()].tolist()
                if by == "user":
                    assert int(top.domain.abs().sum().item()) == 0
                if item_idx is not None:                        # against the helper too: a list repeats no item
                    ref = flat(topk_exact(pred.cpu().numpy(), X[:, 3], 300, X[:, 4] if by == "domain" else None,
                                          3 if by == "domain" else 1, X[:, 1], 5))
                    _same(_got(top, int(top.err.item())), ref, f"{mode} {by}")
        after = ev.test(data)
        assert sorted(after) == sorted(before) and after == before   # recommend() leaves test() as it was: keys and values
    with pytest.raises(ValueError, match="user outside"):
        Evaluator(ple, mode="multi", domain_idx=4, n_domain=3, user_idx=3, n_user=299).recommend(loader)
    with pytest.raises(ValueError, match="domain_idx"):
        Evaluator(ple, mode="multi", user_idx=3, n_user=300).recommend(loader)
    top = Evaluator(ple, mode="multi", user_idx=3, n_user=300).recommend(loader, by="user", k=3)
    assert top.k == 3 and top.item is None and int((top.start[1:] - top.start[:-1]).max().item()) == 3


@pytest.mark.parametrize("with_item", [False, True])
def test_topk_merge_of_three_passes_equals_one_call(cuda, with_item):
    from cdcmdr_amd.evaluate import TopK, eval_topk
    n, n_user, n_domain, k = 6000, 37, 3, 4
    s, u, dom, item = _heavy_ties(n, n_user, n_domain, 71)
    y = np.random.default_rng(72).integers(0, 2, size=n).astype(np.int16)
    pred, label = torch.from_numpy(s).to(cuda), torch.from_numpy(y).to(cuda)
    ut, dt, it = _columns(cuda, u, dom, item if with_item else None, False)
    cuts, acc = [0, 1500, 4100, n], None
    for a, b in zip(cuts, cuts[1:]):
        part = eval_topk(pred[a:b], ut[a:b], n_user, dt[a:b], n_domain, None if it is None else it[a:b], k + (a == 0))
        part.label = label[a:b][part.row.to(torch.int64)]
        acc = part if acc is None else TopK.merge(acc, part, k)
        assert acc.n == b
    one = eval_topk(pred, ut, n_user, dt, n_domain, it, k)
    one.label = label[one.row.to(torch.int64)]
    want = flat(topk_exact(s, u, n_user, dom, n_domain, item if with_item else None, k))
    _same(_got(one, int(one.err.item())), want, "one call")
    acc.rows = one.rows                                         # merge counts the survivors among the kept entries only (documented)
    _equal_topk(acc, one, "merged")
    assert acc.k == k
    row, score = one.dense()
    lists = one.lists()
    assert tuple(row.shape) == (len(want["domain"]), k) and row.dtype == torch.int32 and score.dtype == torch.float32
    row, score = row.cpu().numpy(), score.cpu().numpy()
    for j, (d, usr) in enumerate(zip(want["domain"].tolist(), want["user"].tolist())):
        a, b = want["start"][j], want["start"][j + 1]
        assert row[j, :b - a].tolist() == want["row"][a:b].tolist() and (row[j, b - a:] == -1).all()
        assert score[j, :b - a].view(np.uint32).tolist() == want["score"][a:b].tolist() and np.isnan(score[j, b - a:]).all()
        assert lists[(d, usr)][0] == want["row"][a:b].tolist()
