"""cdc_eval_calibration / eval_calibration / Evaluator(calibration=...) on the device against the exact rationals of
tests/calibration_exact.py (its numpy form; tests/test_calibration_cpu.py holds that to the row-by-row one).

The bounds are derived, not measured.  The kernel's sums are exact integers.  Every double it returns is (an integer numerator ->
double: one rounding, none below 2^53) / (a denominator that is an integer below 2^53 times a power of two: exact): two roundings,
relative (1 + u)^2 - 1 with u = 2^-53; the expected value is the exact rational rounded once more (u / 2).  2.5 u <= the 4 u asked
for: |device - exact| <= 4 * 2^-53 * |exact|.  Counts must be equal, pred_min / pred_max must have the helper's bits, and NaN must
stand exactly where the helper has None."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from calibration_exact import SEGMENT_FIELDS, TABLE_FIELDS, as_float, calibration_exact

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _device(cuda, y, p, K, dom=None, n_domain=1, strided=False):
    """-> ({field: numpy array}, err): the segment fields [n_domain + 1], 'table.<field>' and 'table_q.<field>' [n_domain + 1, K]"""
    from cdcmdr_amd.evaluate import eval_calibration
    n = len(y)
    pred = torch.from_numpy(np.array(p, dtype=np.float32)).to(cuda)
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    dt = None
    if dom is not None and strided:                             # the domain as a column of an [n, 3] id matrix
        X = np.full((n, 3), -7, dtype=np.int32)
        X[:, 1] = dom
        dt = torch.from_numpy(X).to(cuda)[:, 1]
        assert dt.stride(0) == 3
    elif dom is not None:
        dt = torch.from_numpy(np.asarray(dom).astype(np.int32)).to(cuda)
    r = eval_calibration(pred, label, dt, n_domain, K)
    assert r._fields == ("rows", "positives") + SEGMENT_FIELDS + ("table", "table_q")
    assert r.table._fields == r.table_q._fields == TABLE_FIELDS
    out = {}
    for k in ("rows", "positives") + SEGMENT_FIELDS:
        t = getattr(r, k)
        assert t.is_cuda and t.shape == (n_domain + 1,) and t.dtype == (torch.int64 if k in ("rows", "positives") else torch.float64), k
        out[k] = t.cpu().numpy().copy()
    for name, tab in (("table", r.table), ("table_q", r.table_q)):
        for f, t in zip(TABLE_FIELDS, tab):
            want = torch.int64 if f in ("count", "positives") else (torch.float32 if f.startswith("pred_m") else torch.float64)
            assert t.is_cuda and t.shape == (n_domain + 1, K) and t.dtype == want, (name, f)
            out[name + "." + f] = t.cpu().numpy().copy()
    return out, int(eval_calibration.last_err.item())


def _close(got, exact, what):
    if exact is None:
        assert np.isnan(got), (what, got)
        return
    e = float(exact)
    assert abs(got - e) <= 4 * U * abs(e), (what, got, e, abs(got - e), 4 * U * abs(e))     # 2.5 u are due (module docstring)


def _check(got, want, what=""):
    vals, err = got
    assert err == 0, what
    assert vals["rows"].tolist() == [w["rows"] for w in want] and vals["positives"].tolist() == [w["positives"] for w in want], what
    for d, w in enumerate(want):
        for k in SEGMENT_FIELDS:
            print(what, k, d, "device", vals[k][d], "exact", as_float(w[k]))
            _close(vals[k][d], w[k], (what, k, d))
        for name in ("table", "table_q"):
            t = w[name]
            assert vals[name + ".count"][d].tolist() == t["count"], (what, name, d)
            assert vals[name + ".positives"][d].tolist() == t["positives"], (what, name, d)
            for f in ("mean_pred", "pos_rate"):
                for b, e in enumerate(t[f]):
                    _close(vals[name + "." + f][d, b], e, (what, name, f, d, b))
            for f in ("pred_min", "pred_max"):
                exact = np.array([np.nan if v is None else v for v in t[f]], dtype=np.float32)
                dev = vals[name + "." + f][d]
                assert np.array_equal(np.isnan(dev), np.isnan(exact)), (what, name, f, d)
                keep = ~np.isnan(exact)
                assert np.array_equal(dev[keep].view(np.int32), exact[keep].view(np.int32)), (what, name, f, d, dev, exact)


def _same_bits(a, b):
    for k in a[0]:
        x, y = a[0][k], b[0][k]
        if not np.array_equal(x.view(np.int32 if x.dtype == np.float32 else np.int64), y.view(np.int32 if y.dtype == np.float32 else np.int64)):
            return False
    return True


def _ctr_like(rng, n):
    """most mass below 0.1: equal-width bins of very unequal size"""
    p = (rng.random(n) ** 5).astype(np.float32)
    p[rng.random(n) < 0.1] = np.float32(0.03125)                # a tie run
    y = (rng.random(n) < 0.03 + 0.6 * p).astype(np.int16)
    return p, y


def test_one_row_two_rows_and_the_documented_example(cuda):
    for y, p in (([1], [0.25]), ([0], [0.7]), ([0, 1], [0.5, 0.5]), ([1, 0], [0.1, 0.9]), ([1, 1], [0.3, 0.3])):
        for K in (1, 2, 10):
            want = calibration_exact(y, np.array(p, dtype=np.float32), K)
            _check(_device(cuda, y, p, K), want, f"{y}/{p}/{K}")
    # INTEGRATION.md's five rows: dyadic predictions, every figure exact in double
    got, err = _device(cuda, [1, 1, 0, 1, 0], [0.25, 1.0, 0.125, 0.75, 0.25], 2)
    assert err == 0 and got["rows"].tolist() == [5, 5] and got["positives"].tolist() == [3, 3]
    assert got["mean_pred"].tolist() == [0.475] * 2 and got["ctr"].tolist() == [0.6] * 2 and got["brier"].tolist() == [0.140625] * 2
    assert got["pcoc"].tolist() == [2.375 / 3] * 2
    assert got["ece"].tolist() == [0.125] * 2 and got["mce"].tolist() == [0.125] * 2
    assert got["ece_q"].tolist() == [0.275] * 2 and got["mce_q"].tolist() == [1 / 3] * 2
    assert got["table.count"][1].tolist() == [3, 2] and got["table.positives"][1].tolist() == [1, 2]
    assert got["table_q.count"][1].tolist() == [2, 3] and got["table_q.positives"][1].tolist() == [0, 3]
    assert got["table_q.pred_min"][1].tolist() == [0.125, 0.25] and got["table_q.pred_max"][1].tolist() == [0.25, 1.0]


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_small_and_odd_shapes(cuda, n):
    for K in (1, 2, 10):
        rng = np.random.default_rng(100 * n + K)
        p, y = _ctr_like(rng, n)
        dom = rng.integers(0, 2, size=n).astype(np.int32)
        _check(_device(cuda, y, p, K, dom, 2), calibration_exact(y, p, K, dom, 2), f"{n}/{K}")
        _check(_device(cuda, y, p, K), calibration_exact(y, p, K), f"{n}/{K}/no domain")


@pytest.mark.parametrize("K", [10, 16])
def test_edge_values(cuda, K):
    edge = [0.0, -0.0, 1.0, 2.0 ** -40, 1.0 - 2.0 ** -24, 1e-45, 1e-40, 2.0 ** -33, 3 * 2.0 ** -34]
    p = np.array(edge + [b / 10 for b in range(11)] + [b / 16 for b in range(17)], dtype=np.float32)
    p = np.concatenate([p, p, p])
    rng = np.random.default_rng(K)
    y = rng.integers(0, 2, size=len(p)).astype(np.int16)
    dom = rng.integers(0, 2, size=len(p)).astype(np.int32)
    want = calibration_exact(y, p, K, dom, 2)
    got = _device(cuda, y, p, K, dom, 2)
    _check(got, want, f"edges/{K}")
    assert got[0]["table.pred_min"][2, 0] == 0.0 and not np.signbit(got[0]["table.pred_min"][2, 0])      # -0.0 counts as 0
    assert got[0]["table.pred_max"][2, K - 1] == 1.0
    alone = _device(cuda, [1, 0], [2.0 ** -40, 2.0 ** -40], K)                   # quantises to 0: predicted 0 against a CTR of 1/2
    assert alone[0]["mean_pred"].tolist() == [0.0, 0.0] and alone[0]["brier"].tolist() == [0.5, 0.5] and alone[0]["pcoc"].tolist() == [0.0, 0.0]


def test_tie_runs_across_quantile_bounds_and_row_permutations(cuda):
    rng = np.random.default_rng(5)
    n, n_domain, K = 3000, 2, 7
    p = rng.choice(np.array([0.02, 0.05, 0.05, 0.05, 0.2, 0.6], dtype=np.float32), size=n)      # runs of hundreds of rows
    y = (rng.random(n) < 0.4).astype(np.int16)
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    want = calibration_exact(y, p, K, dom, n_domain)
    for w in want:                                                               # most bounds cut a run: the same score on both sides
        assert sum(lo == hi for lo, hi in zip(w["table_q"]["pred_max"][:-1], w["table_q"]["pred_min"][1:])) >= 3
    got = _device(cuda, y, p, K, dom, n_domain)
    _check(got, want, "ties")
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(n)
        assert _same_bits(got, _device(cuda, y[perm], p[perm], K, dom[perm], n_domain, strided=True)), seed


def test_empty_single_class_and_short_segments(cuda):
    rng = np.random.default_rng(9)
    n, n_domain, K = 900, 5, 12
    p, y = _ctr_like(rng, n)
    dom = rng.choice([0, 2, 3], size=n).astype(np.int32)                         # 1 is empty
    y[dom == 2] = 0                                                              # no positive: pcoc NaN
    y[dom == 3] = 1                                                              # no negative: pcoc defined
    dom[:5] = 4                                                                  # 5 rows for 12 bins
    y[:5] = [0, 1, 1, 0, 1]
    want = calibration_exact(y, p, K, dom, n_domain)
    assert want[1]["rows"] == 0 and want[2]["positives"] == 0 and want[3]["positives"] == want[3]["rows"] > 0 and want[4]["rows"] == 5
    assert want[2]["pcoc"] is None and want[3]["pcoc"] is not None and want[2]["ece"] is not None
    got = _device(cuda, y, p, K, dom, n_domain, strided=True)
    _check(got, want, "segments")
    assert np.isnan(got[0]["mean_pred"][1]) and np.isnan(got[0]["table.mean_pred"][1]).all() and not got[0]["table_q.count"][1].any()
    assert _same_bits(got, _device(cuda, y, p, K, dom, n_domain))                # the strided column changes nothing


@functools.lru_cache(maxsize=None)
def _big():
    """70 000 rows over 7 domains of very unequal size, skewed like CTR predictions: the row pass spans many workgroups, and cell
    changes fall inside a wave's round as well as on its ends"""
    n, n_domain = 70_000, 7
    rng = np.random.default_rng(70_000)
    p, y = _ctr_like(rng, n)
    p[:6] = [-0.0, 0.0, 1e-42, 1.0 - 2 ** -24, 1.0, 2.0 ** -40]
    dom = rng.choice(n_domain, size=n, p=[0.5, 0.3, 0.1, 0.05, 0.04, 0.00996, 0.00004]).astype(np.int32)
    dom[dom == 6] = 5
    dom[[10, 20_000, 69_999]] = 6
    for a in (p, y, dom):
        a.setflags(write=False)
    return n_domain, y, p, dom


@pytest.mark.parametrize("K", [10, 15, 1024])
def test_many_workgroups_and_skewed_bins(cuda, K):
    n_domain, y, p, dom = _big()
    want = calibration_exact(y, p, K, dom, n_domain)
    assert want[6]["rows"] == 3 and want[0]["rows"] > 30_000
    if K == 10:
        assert want[n_domain]["table"]["count"][0] > 40_000 > 2_000 > want[n_domain]["table"]["count"][9] > 0      # very unequal
    got = _device(cuda, y, p, K, dom, n_domain, strided=True)
    _check(got, want, f"70k/{K}")
    perm = np.random.default_rng(K).permutation(len(y))
    assert _same_bits(got, _device(cuda, y[perm], p[perm], K, dom[perm], n_domain))


def test_bad_rows_set_the_error_word(cuda):
    p = np.array([0.2, 0.3, 0.7, 0.6, 0.1, 0.4], dtype=np.float32)
    y = [0, 1, 1, 0, 1, 0]
    good = _device(cuda, y, p, 4)
    assert good[1] == 0
    bad = p.copy()
    bad[3] = np.nan
    got = _device(cuda, y, bad, 4)
    assert got[1] == 4 and got[0]["rows"].tolist() == [6, 6] and not np.isnan(got[0]["mean_pred"]).any()      # the launch completes
    bad[3] = 1.5
    got = _device(cuda, y, bad, 4)
    assert got[1] == 4 and got[0]["table.pred_max"][1, 3] == 1.0                 # counted as 1
    bad[3], bad[1] = 0.6, -0.25
    got = _device(cuda, y, bad, 4)
    assert got[1] == 2 and got[0]["table.pred_min"][1, 0] == 0.0                 # counted as 0
    assert _device(cuda, [0, 1, 2, 0, 1, 0], p, 4)[1] == 3                       # label 2
    got = _device(cuda, y, p, 4, dom=[0, 1, 0, 1, 2, 1], n_domain=2)             # domain == n_domain
    assert got[1] == 5 and got[0]["rows"].tolist() == [2, 4, 6]
    assert _device(cuda, y, p, 4, dom=[0, -1, 0, 1, 1, 1], n_domain=2)[1] == 2
    assert _same_bits(good, _device(cuda, y, p, 4))


def test_a_captured_call_replays_to_the_eager_bits(cuda):
    from cdcmdr_amd.evaluate import eval_calibration
    n, n_domain, K = 5000, 3, 10
    data = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        p, y = _ctr_like(rng, n)
        data.append((p, y, rng.integers(0, n_domain, size=n).astype(np.int32)))
    bufs = [torch.from_numpy(a).to(cuda) for a in data[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator
        eval_calibration(bufs[0], bufs[1], bufs[2], n_domain, K)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = eval_calibration(bufs[0], bufs[1], bufs[2], n_domain, K)
        err = eval_calibration.last_err
    for p, y, dom in (data[1], data[0]):
        for t, a in zip(bufs, (p, y, dom)):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        eager, _ = _device(cuda, y, p, K, dom, n_domain)
        for k in ("rows", "positives") + SEGMENT_FIELDS:
            assert np.array_equal(getattr(r, k).cpu().numpy().view(np.int64), eager[k].view(np.int64)), k
        for name, tab in (("table", r.table), ("table_q", r.table_q)):
            for f, t in zip(TABLE_FIELDS, tab):
                a, b = t.cpu().numpy(), eager[name + "." + f]
                w = np.int32 if a.dtype == np.float32 else np.int64
                assert np.array_equal(a.view(w), b.view(w)), (name, f)


def _tiny(cuda):
    from cdcmdr_amd.model.mmoe import MMoE
    FD = [50, 50, 50, 4]                                        # 4 fields of vocabulary <= 50; column 3: 4 domains, 3 of them present
    torch.manual_seed(7)
    model = MMoE(FD, 8, 4, 4, (32, 16), (8,), dropout=0.2).to(cuda).set_precision("f32")
    rng = np.random.default_rng(8)
    n, bs = 600, 256                                            # ragged last batch
    X = np.stack([rng.integers(0, d, size=n) for d in FD], axis=1).astype(np.int32)
    X[X[:, 3] == 2, 3] = 0                                      # domain 2 is absent
    y = rng.integers(0, 2, size=n).astype(np.int16)
    g = X[:, 3].astype(np.int64)
    loader = [(torch.from_numpy(X[i:i + bs]).to(cuda), torch.from_numpy(y[i:i + bs]).to(cuda).reshape(-1, 1),
               torch.from_numpy(g[i:i + bs]).to(cuda).reshape(-1, 1)) for i in range(0, n, bs)]
    return model, loader, X, y


def test_evaluator_calibration(cuda):
    from cdcmdr_amd.evaluate import Evaluator, eval_calibration
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.1, 3: 0.1}
    kw = dict(mode="multi", domain_idx=3, n_domain=4, domain_cnt_weight=w)
    res0 = Evaluator(model, **kw).test(loader)
    assert sorted(res0) == ["domain_auc", "domain_loss", "mean_auc", "mean_loss", "total_auc", "total_loss"]     # calibration=False: today's keys
    names = ("pcoc", "brier", "ece", "ece_quantile")
    for cal, K in ((True, 10), (7, 7)):
        ev = Evaluator(model, calibration=cal, **kw)
        res = ev.test(loader)
        assert sorted(res) == sorted(list(res0) + [pre + k for pre in ("total_", "domain_", "mean_") for k in names])
        for k in res0:
            assert res[k] == res0[k]                            # the other figures are untouched
        pred, label, dom = ev.predict(loader)
        assert np.array_equal(label.cpu().numpy(), y) and np.array_equal(dom.cpu().numpy(), X[:, 3])
        r = eval_calibration(pred, label, dom, 4, K)
        _check(_device(cuda, y, pred.cpu().numpy(), K, X[:, 3], 4), calibration_exact(y, pred.cpu().numpy(), K, X[:, 3], 4), f"evaluator/{K}")
        for k, t in zip(names, (r.pcoc, r.brier, r.ece, r.ece_q)):
            v = t.cpu().tolist()
            assert res["total_" + k] == v[4] and res["domain_" + k] == {0: v[0], 1: v[1], 3: v[3]}      # the absent domain 2 is left out
            assert res["mean_" + k] == sum(w[d] * v[d] for d in (0, 1, 3))
        table, table_q, segments = ev.calibration_table(loader)
        assert segments == [0, 1, 2, 3, "all"]
        for host, devt in ((table, r.table), (table_q, r.table_q)):
            assert host._fields == TABLE_FIELDS
            for f, a, t in zip(TABLE_FIELDS, host, devt):
                b = t.cpu().numpy()
                assert isinstance(a, np.ndarray) and a.shape == (5, K) and a.dtype == b.dtype, f
                vw = np.int32 if a.dtype == np.float32 else np.int64
                assert np.array_equal(a.view(vw), b.view(vw)), f
    # per-domain evaluation off: the totals only, and the table of all rows
    ev = Evaluator(model, mode="multi", domain_idx=3, n_domain=4, is_evaluate_multi_domain=False, calibration=True)
    res1 = ev.test(loader)
    assert sorted(res1) == sorted(["total_auc", "total_loss"] + ["total_" + k for k in names])
    assert all(res1["total_" + k] == res["total_" + k] for k in ("pcoc", "brier")) and res1["total_ece"] != res["total_ece"]      # 10 bins, not 7
    table, table_q, segments = ev.calibration_table(loader)
    assert segments == ["all"] and table.count.shape == (1, 10) and int(table.count.sum()) == int(table_q.count.sum()) == 600
    # a prediction outside [0, 1] names its row
    bad = [(Xb, yb, gb) for Xb, yb, gb in loader]

    class Shifted(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, X):
            out = self.inner(X)
            if X.shape[0] < 256:                                # the last batch: rows 512..599
                out = out.clone()
                out[3] = 1.25
            return out

    with pytest.raises(ValueError, match="row 515: prediction outside"):
        Evaluator(Shifted(model), calibration=True, **kw).test(bad)


def test_abi_bad_arguments_launch_nothing(cuda):
    from cdcmdr_amd import _lib
    lib = _lib.load()
    n, n_domain, K = 100, 3, 5
    seg = n_domain + 1
    pred = torch.rand(n, device=cuda)
    label = torch.zeros(n, dtype=torch.int16, device=cuda)
    dom = torch.zeros(n, dtype=torch.int32, device=cuda)
    seg_out = torch.full((8 * seg,), -3.0, dtype=torch.float64, device=cuda)
    seg_counts = torch.full((2 * seg,), -3, dtype=torch.int64, device=cuda)
    tab_out = torch.full((4 * seg * K,), -3.0, dtype=torch.float64, device=cuda)
    tab_counts = torch.full((4 * seg * K,), -3, dtype=torch.int64, device=cuda)
    tab_range = torch.full((4 * seg * K,), -3.0, dtype=torch.float32, device=cuda)
    err = torch.full((1,), -3, dtype=torch.int32, device=cuda)
    need = lib.cdc_eval_calibration_workspace_bytes(n, n_domain, K)
    assert lib.cdc_eval_calibration_workspace_bytes(n, n_domain, 1024) > need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pred=pred.data_ptr(), label=label.data_ptr(), domain=dom.data_ptr(), n=n, n_domain=n_domain, n_bins=K, ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cdc_eval_calibration(a["pred"], a["label"], a["domain"], 1, a["n"], a["n_domain"], a["n_bins"], seg_out.data_ptr(),
                                        seg_counts.data_ptr(), tab_out.data_ptr(), tab_counts.data_ptr(), tab_range.data_ptr(), err.data_ptr(),
                                        a["ws"], a["ws_bytes"], stream)

    for kw in ({"pred": None}, {"label": None}, {"ws": None}, {"domain": None}, {"n": 0}, {"n_domain": 0}, {"n_bins": 0}, {"n_bins": 1025},
               {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": ws.data_ptr() + 8}):
        assert call(**kw) == -1, kw                             # CDC_E_BADARG
    assert call(n=1 << 31) == -2                                # CDC_E_TOOBIG
    torch.cuda.synchronize()
    assert (seg_out == -3.0).all() and (seg_counts == -3).all() and (tab_out == -3.0).all() and (tab_counts == -3).all()
    assert (tab_range == -3.0).all() and int(err.item()) == -3 and not ws.any()      # nothing ran
    err.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert seg_counts[:seg].tolist() == [n, 0, 0, n] and int(err.item()) == 0
    assert int(tab_counts[:seg * K].sum().item()) == 2 * n and int(tab_counts[2 * seg * K:3 * seg * K].sum().item()) == 2 * n
