"""cdc_eval_rank / eval_rank / Evaluator(rank_at=...) on the device against the exact rationals of tests/rank_exact.py.

The bound is derived, not measured, and it is ABSOLUTE: every figure lies in [0, 1].  With u = 2^-53 and to first order:

  a counted group's figure at cut-off K.  The device reads the same discount table D as the helper, and D[b] - D[a] is one correctly
    rounded subtraction.
      recall, precision   H is an exact integer plus ONE rounded quotient (the tie run that straddles K), their sum and one division: 3.
      ndcg   a run's term is share * (D[b] - D[a]): three roundings, each relative to the term, and the terms add up to at most the
             ideal DCG, so they cost 3 together; at most K - 1 additions of partial sums below the ideal DCG and one division: K + 3.
      mrr    pr_j carries 2 j roundings and pr_j / rank one more, each relative to a term of a sum that is at most sum_j pr_j <= 1 and
             weighted by at most (j + 1) / rank <= 1: 2 together; at most K - 1 additions: K + 1.
      hit    1 - q with q a product of at most K quotients: 2 K roundings relative to q <= 1, and the subtraction: 2 K + 1.
    so at most max(2 K + 1, K + 3) <= 2 K + 3 for any of them;
  the segment's value sum_g w_g m_g / sum_g w_g over G counted groups: one multiplication per term (relative to the term), G - 1
    additions of non-negative terms in numerator and in denominator, one division: 2 G.

The bound used is (2 K + 2 G + 8) u — below the (4 K + 2 G + 16) u a looser count of the per-group roundings gives.  Counts must
be equal, and NaN must stand exactly where the helper counts no group."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from rank_exact import FIGURES, rank_exact

pytestmark = pytest.mark.gpu
EPS = Fraction(1, 2 ** 53)


def _table(k_max):
    from cdcmdr_amd.evaluate import rank_discounts
    return rank_discounts(k_max).numpy()


def _device_rank(cuda, y, s, u, n_user, dom=None, n_domain=1, ks=(10,), w=None, strided=False):
    from cdcmdr_amd.evaluate import eval_rank
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
    r = eval_rank(pred, label, ut, n_user, dt, n_domain, ks, wt)
    for t in r[:5]:
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (len(ks), n_domain + 1)
    assert r.counted.dtype == torch.int64 and r.counted.numel() == r.left_out.numel() == n_domain + 1
    err = int(eval_rank.last_err.item())
    return torch.stack(r[:5]).cpu().numpy(), r.counted.cpu().numpy(), r.left_out.cpu().numpy(), err


def _within(got, exact, K, G):
    return abs(Fraction(float(got)) - exact) <= (2 * K + 2 * G + 8) * EPS


def _check(got, want, ks, what=""):
    figs, c, l, err = got
    vals, counted, left = want[:3]
    assert err == 0, what
    assert c.tolist() == counted and l.tolist() == left, (what, c.tolist(), counted, l.tolist(), left)
    worst = 0.0
    for seg, v in enumerate(vals):
        if v is None:
            assert np.isnan(figs[:, :, seg]).all(), (what, seg, figs[:, :, seg])
            continue
        assert not np.isnan(figs[:, :, seg]).any(), (what, seg, figs[:, :, seg])
        for fi, fig in enumerate(FIGURES):
            for q, K in enumerate(ks):
                g, exact = figs[fi, q, seg], v[fig][q]
                diff = abs(Fraction(float(g)) - exact)
                worst = max(worst, float(diff / ((2 * K + 2 * counted[seg] + 8) * EPS)))
                assert _within(g, exact, K, counted[seg]), (what, seg, fig, K, g, float(exact), float(diff / EPS), counted[seg])
    print(what, "counted", counted, "left out", left, "largest error / bound", worst)


def test_rank_hand_example_and_smallest_inputs(cuda):
    one = np.array([0.3], dtype=np.float32)
    figs, c, l, err = _device_rank(cuda, [1], one, [0], 1, ks=(1,))
    assert (figs == 1.0).all() and c.tolist() == [1, 1] and l.tolist() == [0, 0] and err == 0       # one positive row: everything is 1
    figs, c, l, err = _device_rank(cuda, [0], one, [0], 1, ks=(1,))
    assert np.isnan(figs).all() and c.tolist() == [0, 0] and l.tolist() == [1, 1] and err == 0
    # the hand example of INTEGRATION.md
    s = np.array([0.9, 0.5, 0.5, 0.5, 0.1, 0.3, 0.7], dtype=np.float32)
    y, u = [0, 1, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 1, 1]
    got = _device_rank(cuda, y, s, u, 2, ks=(2, 3))
    _check(got, rank_exact(y, s, u, None, 1, (2, 3), _table(3)), (2, 3), "hand")
    want = [0.444416, 11 / 18, 5 / 12, 5 / 6, 5 / 12]
    assert all(abs(got[0][fi, 0, 1] - v) < 5e-7 for fi, v in enumerate(want)), got[0][:, 0, 1]
    # signed zeros tie: one positive among two rows of one score
    z = np.array([-0.0, 0.0], dtype=np.float32)
    got = _device_rank(cuda, [1, 0], z, [0, 0], 5, ks=(1, 2))
    _check(got, rank_exact([1, 0], z, [0, 0], None, 1, (1, 2), _table(2)), (1, 2), "zeros")
    assert got[0][1, 0, 1] == 0.5 and got[0][3, 0, 1] == 0.5 and got[0][4, 0, 1] == 0.5 and got[0][4, 1, 1] == 0.75
    # two users in two domains
    two = np.array([0.3, 0.7], dtype=np.float32)
    got = _device_rank(cuda, [0, 1], two, [0, 1], 2, dom=[0, 1], n_domain=2, ks=(1,))
    _check(got, rank_exact([0, 1], two, [0, 1], [0, 1], 2, (1,), _table(1)), (1,), "two users")
    assert got[1].tolist() == [0, 1, 1] and got[2].tolist() == [1, 0, 1] and np.isnan(got[0][:, 0, 0]).all()


KS_BIG = (1, 5, 10)


@functools.lru_cache(maxsize=None)
def _big():
    """70 000 rows, 50 000 users (mostly one- and two-row groups), 7 domains: domain 5 empty, domain 2 without a positive."""
    n, n_user, n_domain = 70_000, 50_000, 7
    rng = np.random.default_rng(70_000)
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.3] = np.float32(0.5)
    s[:4] = [-0.0, 0.0, 1e-30, 1.0 - 2 ** -24]
    y = (rng.random(n) < 0.4).astype(np.int16)
    u = rng.integers(0, n_user, size=n).astype(np.int32)
    u[:4] = 17                                                   # the signed zeros in one group
    y[:4] = [1, 0, 0, 1]
    u[4:24] = 18                                                 # one group longer than every K, 14 of its 20 rows tied: a run across ranks 5 and 10
    s[4:18] = np.float32(0.25)
    y[4:24:2] = 1
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    dom[dom == 5] = 4
    dom[:24] = 1
    y[dom == 2] = 0
    w = 0.1 + rng.random(n_user) * 5.0
    for a in (s, y, u, dom, w):
        a.setflags(write=False)
    table = _table(KS_BIG[-1])
    exact = {None: rank_exact(y, s, u, dom, n_domain, KS_BIG, table, None), "w": rank_exact(y, s, u, dom, n_domain, KS_BIG, table, w)}
    return n_user, n_domain, y, s, u, dom, w, exact


@pytest.mark.parametrize("weighted", [False, True])
def test_rank_many_small_groups_strided_columns(cuda, weighted):
    n_user, n_domain, y, s, u, dom, w, exact = _big()
    want = exact["w" if weighted else None]
    vals, counted, left, notes = want
    assert counted[5] == 0 and left[5] == 0 and vals[5] is None            # the empty domain
    assert counted[2] == 0 and left[2] > 0 and vals[2] is None             # the domain without a positive: every user of it left out
    assert counted[n_domain] > 5000
    assert notes[n_domain]["short"] >= 1 and notes[n_domain]["straddle"] >= 1 and notes[n_domain]["no_negative"] >= 1
    _check(_device_rank(cuda, y, s, u, n_user, dom, n_domain, KS_BIG, w if weighted else None, strided=True), want, KS_BIG, f"70k/{weighted}")


def test_rank_is_invariant_to_the_row_order(cuda):
    n_user, n_domain, y, s, u, dom, w, exact = _big()
    perm = np.random.default_rng(1).permutation(len(y))
    for ww in (w, None):
        a = _device_rank(cuda, y, s, u, n_user, dom, n_domain, KS_BIG, ww)
        b = _device_rank(cuda, y[perm], s[perm], u[perm], n_user, dom[perm], n_domain, KS_BIG, ww)
        nan = np.isnan(a[0])
        assert nan.sum() == 2 * 5 * len(KS_BIG) and np.array_equal(a[0].view(np.int64), b[0].view(np.int64))     # bit for bit, NaN included
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_rank_long_group_long_tie_run_and_a_nearly_empty_segment(cuda):
    n, n_user, ks = 20_000, 300, (1, 64, 1024)
    rng = np.random.default_rng(20_000)
    s = rng.random(n).astype(np.float32)
    u = rng.integers(0, n_user, size=n).astype(np.int32)
    u[(u == 123) | (u == 7)] = 124
    pick = rng.permutation(n)
    big, flat, few = pick[:5000], pick[5000:6200], pick[6200:6240]
    u[big] = 123                                                 # one user owns 5 000 rows: its group spans 16 of the 64 slices ...
    s[big[:1500]] = np.float32(0.625)                            # ... 1 500 of them with one score, below ~1 300 distinct ones: the walk ends at its cap
    u[flat] = 7                                                  # a constant predictor: ONE tie run of 1 200 rows covers the whole top K
    s[flat] = np.float32(0.25)
    y = (rng.random(n) < 0.35).astype(np.int16)
    dom = np.zeros(n, dtype=np.int32)
    dom[few] = 1                                                 # a segment of 40 rows: most of its slices are empty
    assert int((u == 123).sum()) == 5000 and int((s[u == 123] > 0.625).sum()) > 1024 and int((u == 7).sum()) == 1200
    table = _table(1024)
    w = 0.5 + rng.random(n_user)
    for ww in (None, w):
        want = rank_exact(y, s, u, dom, 2, ks, table, ww)
        assert 0 < want[1][1] + want[2][1] <= 40
        _check(_device_rank(cuda, y, s, u, n_user, dom, 2, ks, ww), want, ks, "20k")


def test_rank_group_ids_at_the_top_of_the_32_bit_range(cuda):
    n, n_domain, n_user = 4096, 3, 1 << 30                      # (n_domain + 1) * n_user == 2^32 exactly
    rng = np.random.default_rng(4096)
    pool = np.concatenate([[0, 1, n_user - 2, n_user - 1], rng.integers(0, n_user, size=200)]).astype(np.int64)
    u = pool[rng.integers(0, len(pool), size=n)]
    u[:8] = [0, 1, n_user - 2, n_user - 1, 0, 1, n_user - 2, n_user - 1]
    dom = rng.integers(0, n_domain, size=n)
    dom[:8] = [0, 0, 0, 0, 2, 2, 2, 2]
    s = np.round(rng.random(n), 2).astype(np.float32)
    y = rng.integers(0, 2, size=n)
    _check(_device_rank(cuda, y, s, u, n_user, dom, n_domain, KS_BIG, None, strided=True),
           rank_exact(y, s, u, dom, n_domain, KS_BIG, _table(10), None), KS_BIG, "top ids")


def test_rank_flags_bad_rows(cuda):
    s = np.array([0.2, 0.3, 0.7, 0.6, 0.1], dtype=np.float32)
    y, u = [0, 1, 1, 0, 1], [0, 0, 1, 1, 2]
    assert _device_rank(cuda, y, s, u, 3)[3] == 0
    bad = s.copy()
    bad[1] = np.nan
    assert _device_rank(cuda, y, bad, u, 3)[3] == 2
    assert _device_rank(cuda, y, s, [0, 0, 1, 3, 2], 3)[3] == 4                      # user == n_user
    assert _device_rank(cuda, y, s, [0, 0, -1, 1, 2], 3)[3] == 3
    assert _device_rank(cuda, [0, 1, 1, 0, 2], s, u, 3)[3] == 5                      # label 2
    assert _device_rank(cuda, y, s, u, 3, dom=[0, 1, 2, 0, 1], n_domain=2)[3] == 3   # domain == n_domain
    # a clamped user still indexes user_weight inside its bounds (the call must not read past it): it counts as user n_user - 1
    figs, c, l, err = _device_rank(cuda, y, s, [0, 0, 1, 2 ** 31 - 1, 2], 3, ks=(1,), w=[1.0, 2.0, 3.0])
    assert err == 4
    want = rank_exact(y, s, [0, 0, 1, 2, 2], None, 1, (1,), _table(1), [1.0, 2.0, 3.0])
    _check((figs, c, l, 0), want, (1,), "clamped")


def test_rank_replays_from_a_captured_graph(cuda):
    from cdcmdr_amd.evaluate import eval_rank
    n, n_user, n_domain, ks = 3000, 200, 3, (1, 10)
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
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator, the cached tables
        eval_rank(bufs[0], bufs[1], bufs[2], n_user, bufs[3], n_domain, ks, wt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = eval_rank(bufs[0], bufs[1], bufs[2], n_user, bufs[3], n_domain, ks, wt)
        err = eval_rank.last_err
    table = _table(10)
    for data in (second, first):
        for t, a in zip(bufs, data):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        s, y, u, dom = data
        got = (torch.stack(r[:5]).cpu().numpy(), r.counted.cpu().numpy(), r.left_out.cpu().numpy(), int(err.item()))
        _check(got, rank_exact(y, s, u, dom, n_domain, ks, table, w), ks, "graph")


def _new_keys(ks, multi):
    keys = ["total_rank_users"] + [f"total_{f}@{K}" for f in FIGURES for K in ks]
    if multi:
        keys += ["domain_rank_users"] + [f"{p}_{f}@{K}" for p in ("domain", "mean") for f in FIGURES for K in ks]
    return keys


def _check_result(res, want, ks, n_domain, weight, multi=True):
    vals, counted = want[:2]
    assert res["total_rank_users"] == counted[-1]
    for q, K in enumerate(ks):
        for f in FIGURES:
            assert _within(res[f"total_{f}@{K}"], vals[-1][f][q], K, counted[-1]), (f, K)
            if not multi:
                continue
            assert sorted(res[f"domain_{f}@{K}"]) == list(range(n_domain))
            mean = 0
            for d in range(n_domain):
                assert _within(res[f"domain_{f}@{K}"][d], vals[d][f][q], K, counted[d]), (f, K, d)
                mean += weight[d] * res[f"domain_{f}@{K}"][d]
            assert res[f"mean_{f}@{K}"] == mean
    if multi:
        assert res["domain_rank_users"] == {d: counted[d] for d in range(n_domain)}


def test_evaluator_adds_rank_figures_in_multi_and_single_mode(cuda):
    from cdcmdr_amd.evaluate import Evaluator, PlattRecalibration
    from cdcmdr_amd.model.dcn import DCN
    from cdcmdr_amd.model.mmoe import MMoE
    FD = [30, 2000, 7, 300, 3]                                  # column 3: 300 users, column 4: 3 domains
    ks = (1, 10)
    table = _table(10)
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
    uw = 0.25 + rng.random(300)
    for weights in (None, uw):
        kw = dict(mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=300, user_weight=weights)
        res0 = Evaluator(model, **kw).test(loader)
        ev = Evaluator(model, rank_at=ks, **kw)
        res = ev.test(loader)
        assert sorted(res) == sorted(list(res0) + _new_keys(ks, True))       # exactly today's keys plus the new ones
        for k in res0:
            assert res[k] == res0[k]                            # the other figures are untouched, bit for bit
        pred, label, dom = [t.cpu().numpy() for t in ev.predict(loader)]
        _check_result(res, rank_exact(label, pred, X[:, 3], dom, 3, ks, table, weights), ks, 3, w)
    # rank_at as an int; per-domain evaluation off: the total_* keys only
    kw = dict(mode="multi", domain_idx=4, n_domain=3, is_evaluate_multi_domain=False, user_idx=3, n_user=300)
    ev = Evaluator(model, rank_at=10, **kw)
    res = ev.test(loader)
    assert sorted(res) == sorted(list(Evaluator(model, **kw).test(loader)) + _new_keys((10,), False))
    pred = ev.predict(loader)[0].cpu().numpy()
    _check_result(res, rank_exact(y, pred, X[:, 3], None, 1, (10,), table, None), (10,), 1, None, multi=False)
    # a user id outside [0, n_user) is reported as on the GAUC path, not folded into another user
    with pytest.raises(ValueError, match="user outside"):
        Evaluator(model, mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=299, rank_at=ks).test(loader)
    # after a recalibration map: the figures are those of the mapped predictions
    kw = dict(mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=300)
    recal = Evaluator(model, **kw).fit_recalibration(loader, method="platt")
    assert isinstance(recal, PlattRecalibration)
    ev = Evaluator(model, recalibration=recal, rank_at=ks, **kw)
    res = ev.test(loader)
    pred, label, dom = [t.cpu().numpy() for t in ev.predict(loader)]
    _check_result(res, rank_exact(label, pred, X[:, 3], dom, 3, ks, table, None), ks, 3, w)

    # mode "single": batches are (X, y), one output per row
    torch.manual_seed(4)
    dcn = DCN(FD, 8, 2, (16, 8), dropout=0.0).to(cuda).set_precision("f32")
    loader1 = [(a, b) for a, b, _ in loader]
    ev = Evaluator(dcn, mode="single", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=300, rank_at=ks)
    res = ev.test(loader1)
    pred, label, dom = [t.cpu().numpy() for t in ev.predict(loader1)]
    _check_result(res, rank_exact(label, pred, X[:, 3], dom, 3, ks, table, None), ks, 3, w)


def test_evaluator_adds_rank_figures_in_cdc_mode(cuda):
    import types
    from cdcmdr_amd.data import make_domain_loaders
    from cdcmdr_amd.evaluate import Evaluator
    from cdcmdr_amd.model.cdc import CDC
    n_domain, n_cluster, domain_idx, user_idx, bs = 6, 2, 4, 1, 128
    fd = [7, 300, 3, 50, n_domain, 29]
    ks = (1, 10)
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
    ev = Evaluator(cdc, mode="cdc", domain_idx=domain_idx, n_domain=n_domain, domain_cnt_weight=w, user_idx=user_idx, n_user=300, rank_at=ks)
    res = ev.test((loaders, seq))
    pred, label, dom, user = [t.cpu().numpy() for t in ev._score((loaders, seq))]
    _check_result(res, rank_exact(label, pred, user, dom, n_domain, ks, _table(10), None), ks, n_domain, w)
