"""cdc_eval_gauc / eval_gauc / Evaluator(user_idx=...) on the device against the exact rational GAUC of tests/gauc_exact.py.

The bound is derived, not measured.  A counted group's U, P and N are exact integers; its term costs one division (U/(P N)) and
one multiplication (by the weight).  Numerator and denominator are then each a sum of K positive terms in SOME order (at most
K - 1 roundings each, no cancellation), and one division ends it.  To first order that is (K + 1) + (K - 1) + 1 roundings of
2^-53 relative each; the bound used is (2 K + 8) 2^-53 |value| with K the groups counted in that segment.  The counts must be
equal, and NaN must stand exactly where the helper counts no group."""
import functools
import os

import numpy as np
import pytest
import torch

from gauc_exact import as_float, gauc_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EPS = 2.0 ** -53


def _device_gauc(cuda, y, s, u, n_user, dom=None, n_domain=1, w=None, strided=False):
    from cdcmdr_amd.evaluate import eval_gauc
    n = len(y)
    pred = torch.from_numpy(np.asarray(s, dtype=np.float32)).to(cuda)
    label = torch.from_numpy(np.asarray(y).astype(np.int16)).to(cuda)
    if strided:                                                 # user and domain as columns of one [n, 3] id matrix
        X = np.full((n, 3), -7, dtype=np.int32)
        X[:, 2] = u
        X[:, 0] = dom if dom is not None else 0
        Xd = torch.from_numpy(X).to(cuda)
        ut, dt = Xd[:, 2], (Xd[:, 0] if dom is not None else None)
        assert ut.stride(0) == 3
    else:
        ut = torch.from_numpy(np.asarray(u).astype(np.int32)).to(cuda)
        dt = None if dom is None else torch.from_numpy(np.asarray(dom).astype(np.int32)).to(cuda)
    wt = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).to(cuda)
    g, c, l = eval_gauc(pred, label, ut, n_user, dt, n_domain, wt)
    assert g.is_cuda and g.dtype == torch.float64 and c.dtype == torch.int64 and g.numel() == c.numel() == l.numel() == n_domain + 1
    err = int(eval_gauc.last_err.item())
    return g.cpu().numpy(), c.cpu().numpy(), l.cpu().numpy(), err


def _check(got, want, what=""):
    g, c, l, err = got
    vals, counted, left = want
    assert err == 0, what
    print(what, "device", g.tolist(), "exact", [as_float(v) for v in vals], "counted", counted, "left out", left)
    assert c.tolist() == counted and l.tolist() == left, (what, c.tolist(), counted, l.tolist(), left)
    for k, v in enumerate(vals):
        if v is None:
            assert np.isnan(g[k]), (what, k, g[k])
            continue
        exact = float(v)
        bound = (2 * counted[k] + 8) * EPS * abs(exact)
        assert abs(g[k] - exact) <= bound, (what, k, g[k], exact, abs(g[k] - exact), bound)


def test_gauc_golden_g18_both_weightings(cuda):
    d = np.load(os.path.join(GOLD, "g18_gauc.npz"))
    n_domain, n_user = int(d["n_domain"]), int(d["n_user"])
    for tag, w in (("none", None), ("w", d["weights"])):
        got = _device_gauc(cuda, d["targets"], d["scores"], d["users"], n_user, d["domains"], n_domain, w)
        _check(got, gauc_exact(d["targets"], d["scores"], d["users"], d["domains"], n_domain, w), f"g18/{tag}")
        for k in range(n_domain + 1):                            # and the reference's own figures, at the fixture's 1e-12
            ref = float(d[f"gauc_all_{tag}" if k == n_domain else f"gauc_d{k}_{tag}"])
            assert (np.isnan(got[0][k]) and np.isnan(ref)) or abs(got[0][k] - ref) <= 1e-12 * abs(ref), (tag, k, got[0][k], ref)


def test_gauc_smallest_inputs(cuda):
    one = np.array([0.3], dtype=np.float32)
    g, c, l, err = _device_gauc(cuda, [1], one, [0], 1)
    assert np.isnan(g).all() and c.tolist() == [0, 0] and l.tolist() == [1, 1] and err == 0
    two = np.array([0.3, 0.7], dtype=np.float32)
    g, c, l, err = _device_gauc(cuda, [0, 1], two, [4, 4], 5)                       # one user, both classes, ordered
    assert g.tolist() == [1.0, 1.0] and c.tolist() == [1, 1] and l.tolist() == [0, 0] and err == 0
    g, c, l, err = _device_gauc(cuda, [1, 0], two, [4, 4], 5, w=[1.5, 1.5, 1.5, 1.5, 0.3])
    assert g.tolist() == [0.0, 0.0] and c.tolist() == [1, 1]
    g, c, l, err = _device_gauc(cuda, [1, 0], np.array([-0.0, 0.0], dtype=np.float32), [0, 0], 5)    # signed zeros tie
    assert g.tolist() == [0.5, 0.5]
    g, c, l, err = _device_gauc(cuda, [0, 1], two, [0, 1], 2, dom=[0, 1], n_domain=2)               # two users: nothing countable
    assert np.isnan(g).all() and c.tolist() == [0, 0, 0] and l.tolist() == [1, 1, 2] and err == 0


@functools.lru_cache(maxsize=None)
def _big():
    """70 000 rows, 50 000 users (mostly one- and two-row groups), 7 domains: domain 5 empty, domain 2 single-class."""
    n, n_user, n_domain = 70_000, 50_000, 7
    rng = np.random.default_rng(70_000)
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.3] = np.float32(0.5)
    s[:4] = [-0.0, 0.0, 1e-30, 1.0 - 2 ** -24]
    y = (rng.random(n) < 0.4).astype(np.int16)
    u = rng.integers(0, n_user, size=n).astype(np.int32)
    u[:4] = 17                                                   # the signed zeros in one group
    y[:4] = [1, 0, 0, 1]
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    dom[dom == 5] = 4
    dom[:4] = 1
    y[dom == 2] = 0
    w = 0.1 + rng.random(n_user) * 5.0
    for a in (s, y, u, dom, w):
        a.setflags(write=False)
    exact = {None: gauc_exact(y, s, u, dom, n_domain, None), "w": gauc_exact(y, s, u, dom, n_domain, w)}
    return n_user, n_domain, y, s, u, dom, w, exact


@pytest.mark.parametrize("weighted", [False, True])
def test_gauc_many_small_groups_strided_columns(cuda, weighted):
    n_user, n_domain, y, s, u, dom, w, exact = _big()
    want = exact["w" if weighted else None]
    assert want[1][5] == 0 and want[2][5] == 0 and want[0][5] is None      # the empty domain
    assert want[1][2] == 0 and want[2][2] > 0 and want[0][2] is None       # the single-class domain
    assert want[1][n_domain] > 5000
    _check(_device_gauc(cuda, y, s, u, n_user, dom, n_domain, w if weighted else None, strided=True), want, f"70k/{weighted}")


def test_gauc_is_invariant_to_the_row_order(cuda):
    n_user, n_domain, y, s, u, dom, w, exact = _big()
    a = _device_gauc(cuda, y, s, u, n_user, dom, n_domain, w)
    perm = np.random.default_rng(1).permutation(len(y))
    b = _device_gauc(cuda, y[perm], s[perm], u[perm], n_user, dom[perm], n_domain, w)
    nan = np.isnan(a[0])
    assert nan.sum() == 2 and np.array_equal(a[0].view(np.int64), b[0].view(np.int64))           # bit for bit, NaN included
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    c = _device_gauc(cuda, y, s, u, n_user, dom, n_domain, None)
    d = _device_gauc(cuda, y[perm], s[perm], u[perm], n_user, dom[perm], n_domain, None)
    assert np.array_equal(c[0].view(np.int64), d[0].view(np.int64))


def test_gauc_group_and_tie_run_longer_than_a_tile(cuda):
    n, n_user = 20_000, 300
    rng = np.random.default_rng(20_000)
    s = rng.random(n).astype(np.float32)
    u = rng.integers(0, n_user, size=n).astype(np.int32)
    u[u == 123] = 124
    big = rng.permutation(n)[:5000]
    u[big] = 123                                                 # one user owns 5 000 rows ...
    s[big[:1500]] = np.float32(0.625)                            # ... 30 % of them with one score
    y = (rng.random(n) < 0.35).astype(np.int16)
    assert int((u == 123).sum()) == 5000
    w = 0.5 + rng.random(n_user)
    for ww in (None, w):
        _check(_device_gauc(cuda, y, s, u, n_user, None, 1, ww), gauc_exact(y, s, u, None, 1, ww), "20k")


def test_gauc_group_ids_at_the_top_of_the_32_bit_range(cuda):
    n, n_domain, n_user = 4096, 3, 1 << 30                      # (n_domain + 1) * n_user == 2^32 exactly
    rng = np.random.default_rng(4096)
    pool = np.concatenate([[0, 1, n_user - 2, n_user - 1], rng.integers(0, n_user, size=200)]).astype(np.int64)
    u = pool[rng.integers(0, len(pool), size=n)]
    u[:8] = [0, 1, n_user - 2, n_user - 1, 0, 1, n_user - 2, n_user - 1]
    dom = rng.integers(0, n_domain, size=n)
    dom[:8] = [0, 0, 0, 0, 2, 2, 2, 2]
    s = np.round(rng.random(n), 2).astype(np.float32)
    y = rng.integers(0, 2, size=n)
    _check(_device_gauc(cuda, y, s, u, n_user, dom, n_domain, None, strided=True), gauc_exact(y, s, u, dom, n_domain, None), "top ids")


def test_gauc_flags_bad_rows(cuda):
    s = np.array([0.2, 0.3, 0.7, 0.6, 0.1], dtype=np.float32)
    y, u = [0, 1, 1, 0, 1], [0, 0, 1, 1, 2]
    assert _device_gauc(cuda, y, s, u, 3)[3] == 0
    bad = s.copy()
    bad[1] = np.nan
    assert _device_gauc(cuda, y, bad, u, 3)[3] == 2
    assert _device_gauc(cuda, y, s, [0, 0, 1, 3, 2], 3)[3] == 4                      # user == n_user
    assert _device_gauc(cuda, y, s, [0, 0, -1, 1, 2], 3)[3] == 3
    assert _device_gauc(cuda, [0, 1, 1, 0, 2], s, u, 3)[3] == 5                      # label 2
    assert _device_gauc(cuda, y, s, u, 3, dom=[0, 1, 2, 0, 1], n_domain=2)[3] == 3   # domain == n_domain
    # a clamped user still indexes user_weight inside its bounds (the call must not read past it)
    assert _device_gauc(cuda, y, s, [0, 0, 1, 2 ** 31 - 1, 2], 3, w=[1.0, 2.0, 3.0])[3] == 4


def test_gauc_replays_from_a_captured_graph(cuda):
    from cdcmdr_amd.evaluate import eval_gauc
    n, n_user, n_domain = 3000, 200, 3
    rng = np.random.default_rng(9)

    def draw():
        return (np.round(rng.random(n), 2).astype(np.float32), rng.integers(0, 2, size=n).astype(np.int16),
                rng.integers(0, n_user, size=n).astype(np.int32), rng.integers(0, n_domain, size=n).astype(np.int32))
    first, second = draw(), draw()
    w = 0.25 + rng.random(n_user)
    bufs = [torch.from_numpy(a).to(cuda) for a in first]
    wt = torch.from_numpy(w).to(cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator
        eval_gauc(bufs[0], bufs[1], bufs[2], n_user, bufs[3], n_domain, wt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g, c, l = eval_gauc(bufs[0], bufs[1], bufs[2], n_user, bufs[3], n_domain, wt)
        err = eval_gauc.last_err
    for data in (second, first):
        for t, a in zip(bufs, data):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        s, y, u, dom = data
        _check((g.cpu().numpy(), c.cpu().numpy(), l.cpu().numpy(), int(err.item())), gauc_exact(y, s, u, dom, n_domain, w), "graph")


def _close(a, v, k):
    return abs(a - float(v)) <= (2 * k + 8) * EPS * abs(float(v))


def test_evaluator_adds_gauc_in_multi_and_single_mode(cuda):
    from cdcmdr_amd.evaluate import Evaluator
    from cdcmdr_amd.model.dcn import DCN
    from cdcmdr_amd.model.mmoe import MMoE
    FD = [30, 2000, 7, 300, 3]                                  # column 3: 300 users, column 4: 3 domains
    torch.manual_seed(3)
    model = MMoE(FD, 8, 3, 4, (32, 16), (8,), dropout=0.2).to(cuda).set_precision("f32")
    rng = np.random.default_rng(5)
    n, bs = 2500, 1024                                          # ragged last batch
    X = np.stack([rng.integers(0, d, size=n) for d in FD], axis=1).astype(np.int32)
    y = rng.integers(0, 2, size=n).astype(np.int16)
    g = X[:, 4].astype(np.int64)
    loader = [(torch.from_numpy(X[i:i + bs]).to(cuda), torch.from_numpy(y[i:i + bs]).to(cuda).reshape(-1, 1),
               torch.from_numpy(g[i:i + bs]).to(cuda).reshape(-1, 1)) for i in range(0, n, bs)]
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    base = Evaluator(model, mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w)
    res0 = base.test(loader)
    assert sorted(res0) == ["domain_auc", "domain_loss", "mean_auc", "mean_loss", "total_auc", "total_loss"]     # user_idx=None: today's keys
    uw = 0.25 + rng.random(300)
    for weights in (None, uw):
        ev = Evaluator(model, mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=300, user_weight=weights)
        res = ev.test(loader)
        out = ev.predict(loader)
        assert len(out) == 3                                    # predict() keeps its three-tuple
        pred, label, dom = [t.cpu().numpy() for t in out]
        assert np.array_equal(dom, X[:, 4]) and np.array_equal(label, y)
        vals, counted, _ = gauc_exact(label, pred, X[:, 3], dom, 3, weights)
        assert sorted(res) == sorted(list(res0) + ["total_gauc", "domain_gauc", "mean_gauc"])
        for k in res0:
            assert res[k] == res0[k]                            # the other figures are untouched
        assert _close(res["total_gauc"], vals[3], counted[3])
        assert sorted(res["domain_gauc"]) == [0, 1, 2]
        mean = 0
        for d in range(3):
            assert _close(res["domain_gauc"][d], vals[d], counted[d])
            mean += w[d] * res["domain_gauc"][d]
        assert res["mean_gauc"] == mean
    # per-domain evaluation off: total_gauc only
    ev = Evaluator(model, mode="multi", domain_idx=4, n_domain=3, is_evaluate_multi_domain=False, user_idx=3, n_user=300)
    res = ev.test(loader)
    assert sorted(res) == ["total_auc", "total_gauc", "total_loss"]
    pred = ev.predict(loader)[0].cpu().numpy()
    vals, counted, _ = gauc_exact(y, pred, X[:, 3], None, 1, None)
    assert _close(res["total_gauc"], vals[1], counted[1])
    # a user id outside [0, n_user) is reported, not folded into another user
    with pytest.raises(ValueError, match="user outside"):
        Evaluator(model, mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=299).test(loader)

    # mode "single": batches are (X, y), one output per row
    torch.manual_seed(4)
    dcn = DCN(FD, 8, 2, (16, 8), dropout=0.0).to(cuda).set_precision("f32")
    loader1 = [(a, b) for a, b, _ in loader]
    ev = Evaluator(dcn, mode="single", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=300)
    res = ev.test(loader1)
    pred, label, dom = [t.cpu().numpy() for t in ev.predict(loader1)]
    vals, counted, _ = gauc_exact(label, pred, X[:, 3], dom, 3, None)
    assert _close(res["total_gauc"], vals[3], counted[3]) and all(_close(res["domain_gauc"][d], vals[d], counted[d]) for d in range(3))
    assert sorted(Evaluator(dcn, mode="single").test(loader1)) == ["total_auc", "total_loss"]


def test_evaluator_adds_gauc_in_cdc_mode(cuda):
    import types
    from cdcmdr_amd.data import make_domain_loaders
    from cdcmdr_amd.evaluate import Evaluator
    from cdcmdr_amd.model.cdc import CDC
    n_domain, n_cluster, domain_idx, user_idx, bs = 6, 2, 4, 1, 128
    fd = [7, 300, 3, 50, n_domain, 29]
    rng = np.random.default_rng(0)
    n = 1500
    Xn = np.stack([rng.integers(0, d, size=n) for d in fd], axis=1).astype(np.int32)
    yn = rng.integers(0, 2, size=(n, 1)).astype(np.int16)
    np.random.seed(1)
    torch.manual_seed(1)
    loaders, seq, w = make_domain_loaders(torch.from_numpy(Xn), torch.from_numpy(yn), bs, cuda, domain_idx, n_domain, shuffle=False)
    cfg = types.SimpleNamespace(mmoe_n_expert=3, dataset_name="t", p_weight=0.5, p_weight_method="linear_decay", p_weight_exp_decay=0.9,
                                old_matrix_weight=0.3, affinity_func="minus", use_atten=False)
    cdc = CDC(fd, 4, n_cluster, n_domain, "mmoe", (16, 8), (8,), domain_idx, domain_cnt_weight=w, n_causal_mask=3, use_metric="loss",
              device=cuda, dropout=0.2, config=cfg).to(cuda).set_precision("f32")
    d2g = [0, 1, 1, 0, 1, 0]
    cdc.domain2group.copy_(torch.tensor(d2g))
    cdc.domain2group_list = list(d2g)
    ev = Evaluator(cdc, mode="cdc", domain_idx=domain_idx, n_domain=n_domain, domain_cnt_weight=w, user_idx=user_idx, n_user=300)
    res = ev.test((loaders, seq))
    pred, label, dom, user = [t.cpu().numpy() for t in ev._score((loaders, seq))]
    assert pred.size == n and sorted(zip(dom.tolist(), user.tolist())) == sorted(zip(Xn[:, domain_idx].tolist(), Xn[:, user_idx].tolist()))
    vals, counted, _ = gauc_exact(label, pred, user, dom, n_domain, None)
    assert _close(res["total_gauc"], vals[n_domain], counted[n_domain])
    mean = 0
    for d in range(n_domain):
        assert _close(res["domain_gauc"][d], vals[d], counted[d])
        mean += w[d] * res["domain_gauc"][d]
    assert res["mean_gauc"] == mean
