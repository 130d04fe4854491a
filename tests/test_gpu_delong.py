"""cdc_eval_auc_delong / eval_auc_ci / Evaluator(auc_ci=True) / Evaluator.compare on the device against the exact rationals of
tests/delong_exact.py (its sorted form; tests/test_delong_cpu.py holds that to the brute-force one).

The bounds are derived, not measured.  The kernel's sums are exact integers, and so are the numerators P sum a^2 - (sum a)^2 and
the denominators P (P-1) 4 N^2 (128-bit).  What is rounded:
  a variance   numerator -> double (1), denominator -> double (1), their quotient (1), the division by P resp. N (1; P and N are
               exact doubles): 4 roundings per term, both terms >= 0, and their sum (1): 5 roundings, i.e. relative (1 + u)^5 - 1
               with u = 2^-53; the expected value is the exact rational rounded once more (u / 2).  5.5 u <= the 16 u asked for:
               |got - want| <= 16 * 2^-53 * want.
  auc, delta   sum -> double (1; exact below 2^53), P * N (1), the quotient (1); the halving is exact: 3 roundings + u / 2 for the
               expected value, held to 4 u.
Counts must be equal, and NaN must stand exactly where the helper has None."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from delong_exact import as_float, delong_exact

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
UNPAIRED = ("auc", "var")
PAIRED = ("auc", "var", "auc_b", "var_b", "delta", "var_delta")


def _device(cuda, y, s, sb=None, dom=None, n_domain=1, strided=False):
    """-> ({field: float64 [n_domain + 1]}, rows, positives, err)"""
    from cdcmdr_amd.evaluate import eval_auc_ci
    n = len(y)
    pred = torch.from_numpy(np.array(s, dtype=np.float32)).to(cuda)
    pb = None if sb is None else torch.from_numpy(np.array(sb, dtype=np.float32)).to(cuda)
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    dt = None
    if dom is not None and strided:                             # the domain as a column of an [n, 4] id matrix
        X = np.full((n, 4), -7, dtype=np.int32)
        X[:, 2] = dom
        dt = torch.from_numpy(X).to(cuda)[:, 2]
        assert dt.stride(0) == 4
    elif dom is not None:
        dt = torch.from_numpy(np.asarray(dom).astype(np.int32)).to(cuda)
    r = eval_auc_ci(pred, label, dt, n_domain, pred_b=pb)
    assert r._fields == (("auc", "var", "rows", "positives") + (PAIRED[2:] if sb is not None else ()))
    for t in r:
        assert t.is_cuda and t.numel() == n_domain + 1
    assert r.auc.dtype == r.var.dtype == torch.float64 and r.rows.dtype == r.positives.dtype == torch.int64
    err = int(eval_auc_ci.last_err.item())
    vals = {k: getattr(r, k).cpu().numpy().copy() for k in (PAIRED if sb is not None else UNPAIRED)}
    return vals, r.rows.cpu().numpy().copy(), r.positives.cpu().numpy().copy(), err


def _check(got, want, what=""):
    vals, rows, pos, err = got
    assert err == 0, what
    assert rows.tolist() == [w["rows"] for w in want] and pos.tolist() == [w["P"] for w in want], (what, rows, pos)
    for k, arr in vals.items():
        for d, w in enumerate(want):
            print(what, k, d, "device", arr[d], "exact", as_float(w[k]))
            if w[k] is None:
                assert np.isnan(arr[d]), (what, k, d, arr[d])
                continue
            exact = float(w[k])
            bound = (16 if "var" in k else 4) * U * abs(exact)          # 5.5 u resp. 3.5 u are due (module docstring)
            assert abs(arr[d] - exact) <= bound, (what, k, d, arr[d], exact, abs(arr[d] - exact), bound)


def _same_bits(a, b):
    return all(np.array_equal(a[0][k].view(np.int64), b[0][k].view(np.int64)) for k in a[0]) and \
        np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _scores(kind, n, rng):
    if kind == "five":
        return rng.choice(np.array([0.1, 0.25, 0.5, 0.75, 0.9], dtype=np.float32), size=n)        # long tie runs
    if kind == "distinct":
        return rng.permutation(n).astype(np.float32) / np.float32(n + 1)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, 0.5, -0.5], dtype=np.float32)     # signed zeros, denormals
    return rng.choice(pool, size=n)


@pytest.mark.parametrize("n", [1, 2, 3, 65, 257, 4099])
def test_small_and_odd_shapes(cuda, n):
    from cdcmdr_amd.evaluate import eval_metrics
    for q, kind in enumerate(("five", "distinct", "zeros")):
        rng = np.random.default_rng(1000 * n + q)
        s, sb = _scores(kind, n, rng), _scores(kind, n, rng)
        y = (rng.random(n) < 0.45).astype(np.int16)
        dom = rng.choice([0, 2], size=n).astype(np.int32)                    # 3 domains: 1 is empty ...
        y[dom == 2] = 1                                                         # ... and 2 holds one class
        want = delong_exact(y, s, sb, dom, 3)
        assert want[1]["rows"] == 0 and want[2]["N"] == 0
        got = _device(cuda, y, s, sb, dom, 3, strided=True)
        _check(got, want, f"{kind}/{n}/paired")
        one = _device(cuda, y, s, None, dom, 3, strided=True)
        _check(one, want, f"{kind}/{n}")
        assert all(np.array_equal(one[0][k].view(np.int64), got[0][k].view(np.int64)) for k in UNPAIRED)      # pred_b changes nothing of a's
        # auc: cdc_eval_metrics' figure, bit for bit
        X = torch.from_numpy(np.stack([dom] * 4, axis=1).astype(np.int32)).to(cuda)
        auc = eval_metrics(torch.from_numpy(s).to(cuda), torch.from_numpy(y).to(cuda), X[:, 1], 3)[0].cpu().numpy()
        assert np.array_equal(auc.view(np.int64), got[0]["auc"].view(np.int64)), (kind, n, auc, got[0]["auc"])
    # no domain column: the one domain is every row
    want = delong_exact(y, s, sb)
    _check(_device(cuda, y, s, sb), want, f"{n}/no domain")


def test_the_documented_example(cuda):
    from cdcmdr_amd.evaluate import eval_auc_ci
    r = eval_auc_ci(torch.tensor([0.9, 0.5, 0.4, 0.1, 0.4], device=cuda), torch.tensor([1, 0, 1, 0, 0], device=cuda))
    assert r.rows.tolist() == [5, 5] and r.positives.tolist() == [2, 2] and int(eval_auc_ci.last_err.item()) == 0
    assert r.auc.tolist() == [0.75, 0.75]
    # S10 / P = 1/16 and S01 / N = 1/48: the first is exact, the second and the sum round once each
    assert all(abs(v - 1 / 12) <= 16 * U / 12 for v in r.var.tolist())


@functools.lru_cache(maxsize=None)
def _big():
    """70 001 rows, 7 domains of very unequal size (one empty, one of 3 rows): segments cross the sort's, the scan's and the reduce
    launch's block boundaries.  The second vector: the first with 300 rows nudged."""
    n, n_domain = 70_001, 7
    rng = np.random.default_rng(70_001)
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.2] = np.float32(0.5)
    s[:4] = [-0.0, 0.0, 1e-42, 1.0 - 2 ** -24]
    y = (rng.random(n) < 0.3 + 0.3 * s).astype(np.int16)
    dom = rng.choice(n_domain, size=n, p=[0.55, 0.3, 0.1, 0.04, 0.0, 0.00996, 0.00004]).astype(np.int32)
    dom[dom == 6] = 5
    dom[[10, 20_000, 70_000]] = 6
    y[[10, 20_000, 70_000]] = [0, 1, 0]
    sb = s.copy()
    hit = rng.permutation(n)[:300]
    sb[hit] += (rng.random(300).astype(np.float32) - np.float32(0.5)) * np.float32(0.02)
    for a in (s, sb, y, dom):
        a.setflags(write=False)
    return n_domain, y, s, sb, dom, delong_exact(y, s, sb, dom, n_domain)


def test_segments_across_block_boundaries_and_the_paired_variance(cuda):
    from cdcmdr_amd.evaluate import eval_metrics
    n_domain, y, s, sb, dom, want = _big()
    assert want[4]["rows"] == 0 and want[6]["rows"] == 3 and want[0]["rows"] > 35_000
    # the paired variance is far below either AUC's own: var_a + var_b - 2 cov would have to cancel at least three of its digits,
    # i.e. carry an error of 1e3 * 5 u relative to the result — the bound below can only be met by the form on the differences
    for d in (0, 1, 2, n_domain):
        assert 0 < want[d]["var_delta"] < want[d]["var"] / 1000, (d, float(want[d]["var_delta"]), float(want[d]["var"]))
    got = _device(cuda, y, s, sb, dom, n_domain, strided=True)
    _check(got, want, "70k")
    auc = eval_metrics(torch.from_numpy(s).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(dom).to(cuda), n_domain)[0].cpu().numpy()
    assert np.array_equal(auc.view(np.int64), got[0]["auc"].view(np.int64))
    # two runs, and the rows in another order: the same bits (NaN included)
    assert _same_bits(got, _device(cuda, y, s, sb, dom, n_domain, strided=True))
    perm = np.random.default_rng(1).permutation(len(y))
    assert _same_bits(got, _device(cuda, y[perm], s[perm], sb[perm], dom[perm], n_domain))
    assert np.isnan(got[0]["var"]).sum() == 2 and np.isnan(got[0]["auc"]).sum() == 1
    # the second vector equal to the first: zero, not merely small
    same = _device(cuda, y, s, s.copy(), dom, n_domain)
    for d in range(n_domain + 1):
        if want[d]["var"] is not None:
            assert same[0]["var_delta"][d] == 0.0 and same[0]["delta"][d] == 0.0
    assert np.array_equal(same[0]["var_b"].view(np.int64), same[0]["var"].view(np.int64))


def test_bad_rows_set_the_error_word(cuda):
    s = np.array([0.2, 0.3, 0.7, 0.6, 0.1], dtype=np.float32)
    y = [0, 1, 1, 0, 1]
    assert _device(cuda, y, s, s)[3] == 0
    bad = s.copy()
    bad[3] = np.nan
    assert _device(cuda, y, s, bad)[3] == 4                                     # a NaN in pred_b alone
    assert _device(cuda, y, bad, s)[3] == 4 and _device(cuda, y, bad)[3] == 4
    assert _device(cuda, [0, 1, 2, 0, 1], s)[3] == 3                             # label 2
    assert _device(cuda, y, s, s, dom=[0, 1, 0, 1, 2], n_domain=2)[3] == 5       # domain == n_domain
    assert _device(cuda, y, s, None, dom=[0, -1, 0, 1, 1], n_domain=2)[3] == 2


def test_sums_of_squares_beyond_64_bits(cuda):
    """3.6 M rows, half of them positive, nearly separable: a positive's placement is close to 2 N = 3.6e6 and the 1.8e6 squares add
    up to 2.3e19 > 2^64 = 1.8e19 — the smallest evaluation set at which a 64-bit sum of squares wraps."""
    n = 3_600_000
    rng = np.random.default_rng(36)
    s = rng.random(n).astype(np.float32)
    y = (s > 0.5).astype(np.int16)
    flip = rng.random(n) < 0.002
    y[flip] ^= 1
    sb = s.copy()
    sb[:1000] = rng.random(1000).astype(np.float32)
    want = delong_exact(y, s, sb)
    assert want[1]["sums"][1] > 1 << 64 and want[1]["sums"][3] > 1 << 64 and want[1]["sums"][0] < 1 << 53
    assert want[1]["auc"] > 0.99
    _check(_device(cuda, y, s, sb), want, "3.6M")


def _tiny(cuda):
    from cdcmdr_amd.model.mmoe import MMoE
    FD = [50, 50, 50, 3]                                        # 4 fields of vocabulary <= 50; column 3: 3 domains
    torch.manual_seed(7)
    model = MMoE(FD, 8, 3, 4, (32, 16), (8,), dropout=0.2).to(cuda).set_precision("f32")
    rng = np.random.default_rng(8)
    n, bs = 600, 256                                            # ragged last batch
    X = np.stack([rng.integers(0, d, size=n) for d in FD], axis=1).astype(np.int32)
    y = rng.integers(0, 2, size=n).astype(np.int16)
    g = X[:, 3].astype(np.int64)
    loader = [(torch.from_numpy(X[i:i + bs]).to(cuda), torch.from_numpy(y[i:i + bs]).to(cuda).reshape(-1, 1),
               torch.from_numpy(g[i:i + bs]).to(cuda).reshape(-1, 1)) for i in range(0, n, bs)]
    return model, loader, X, y


def test_evaluator_auc_ci(cuda):
    from cdcmdr_amd.evaluate import Evaluator
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    res0 = Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w).test(loader)
    assert sorted(res0) == ["domain_auc", "domain_loss", "mean_auc", "mean_loss", "total_auc", "total_loss"]     # auc_ci=False: today's keys
    ev = Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w, auc_ci=True)
    res = ev.test(loader)
    assert sorted(res) == sorted(list(res0) + ["total_auc_se", "domain_auc_se", "mean_auc_se"])
    for k in res0:
        assert res[k] == res0[k]                                # the other figures are untouched
    pred, label, dom = [t.cpu().numpy() for t in ev.predict(loader)]
    assert np.array_equal(label, y) and np.array_equal(dom, X[:, 3])
    want = delong_exact(label, pred, None, dom, 3)
    assert sorted(res["domain_auc_se"]) == [0, 1, 2]
    for d, se in list(res["domain_auc_se"].items()) + [(3, res["total_auc_se"])]:
        exact = math.sqrt(float(want[d]["var"]))                # the square root halves the variance's relative error and rounds once
        assert 0 < se and abs(se - exact) <= 16 * U * exact, (d, se, exact)
    # the formula on the host, from the reported standard errors: se^2 returns to var within 2.5 u, the sum and the root add 2 u
    host = math.sqrt(sum(w[d] ** 2 * res["domain_auc_se"][d] ** 2 for d in range(3)))
    assert abs(res["mean_auc_se"] - host) <= 8 * U * host, (res["mean_auc_se"], host)
    # per-domain evaluation off: the total only
    res = Evaluator(model, mode="multi", domain_idx=3, n_domain=3, is_evaluate_multi_domain=False, auc_ci=True).test(loader)
    assert sorted(res) == ["total_auc", "total_auc_se", "total_loss"]
    assert abs(res["total_auc_se"] - math.sqrt(float(want[3]["var"]))) <= 16 * U * res["total_auc_se"]


def test_evaluator_compare(cuda):
    from cdcmdr_amd.evaluate import Evaluator
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    ev = Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w)
    res = ev.compare(Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w), loader)
    assert sorted(res) == ["domain_delta", "domain_delta_se", "domain_z", "mean_delta", "mean_delta_se", "mean_z",
                           "total_delta", "total_delta_se", "total_z"]
    assert res["total_delta"] == 0.0 and res["total_delta_se"] == 0.0 and math.isnan(res["total_z"])
    assert res["mean_delta"] == 0.0 and res["mean_delta_se"] == 0.0 and math.isnan(res["mean_z"])
    for d in range(3):
        assert res["domain_delta"][d] == 0.0 and res["domain_delta_se"][d] == 0.0 and math.isnan(res["domain_z"][d])

    # the same module under the other precision: scored one pass after the other, the module's own precision is put back
    other = Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w, precision="bf16")
    res = ev.compare(other, loader)
    assert model.precision == "f32"
    pa, label, dom = [t.cpu().numpy() for t in ev.predict(loader)]
    pb = other.predict(loader)[0].cpu().numpy()
    assert model.precision == "f32" and not np.array_equal(pa, pb)
    want = delong_exact(label, pa, pb, dom, 3)
    for d, (delta, se) in enumerate([(res["domain_delta"][k], res["domain_delta_se"][k]) for k in range(3)] + [(res["total_delta"], res["total_delta_se"])]):
        assert abs(delta - float(want[d]["delta"])) <= 4 * U * abs(float(want[d]["delta"])), (d, delta, float(want[d]["delta"]))
        exact = math.sqrt(float(want[d]["var_delta"]))
        assert abs(se - exact) <= 16 * U * exact, (d, se, exact)
    assert res["total_z"] == res["total_delta"] / res["total_delta_se"]
    assert res["mean_delta"] == sum(w[d] * res["domain_delta"][d] for d in range(3))
    host = math.sqrt(sum(w[d] ** 2 * res["domain_delta_se"][d] ** 2 for d in range(3)))
    assert abs(res["mean_delta_se"] - host) <= 8 * U * host and res["mean_z"] == res["mean_delta"] / res["mean_delta_se"]

    # a loader whose second pass yields other labels
    class Reshuffling:
        def __init__(self):
            self.passes = 0

        def __iter__(self):
            self.passes += 1
            if self.passes == 1:
                return iter(loader)
            return iter([(a, 1 - b, c) for a, b, c in loader])

    with pytest.raises(ValueError, match="different labels"):
        ev.compare(Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w), Reshuffling())


def test_abi_bad_arguments_launch_nothing(cuda):
    from cdcmdr_amd import _lib
    lib = _lib.load()
    n, n_domain = 100, 3
    pred = torch.rand(n, device=cuda)
    label = torch.zeros(n, dtype=torch.int16, device=cuda)
    dom = torch.zeros(n, dtype=torch.int32, device=cuda)
    out = torch.full((6 * (n_domain + 1),), -3.0, dtype=torch.float64, device=cuda)
    counts = torch.full((2 * (n_domain + 1),), -3, dtype=torch.int64, device=cuda)
    err = torch.full((1,), -3, dtype=torch.int32, device=cuda)
    need = lib.cdc_eval_auc_delong_workspace_bytes(n, n_domain, 1)
    assert need > lib.cdc_eval_auc_delong_workspace_bytes(n, n_domain, 0) > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pred_a=pred.data_ptr(), pred_b=pred.data_ptr(), label=label.data_ptr(), domain=dom.data_ptr(), n=n, n_domain=n_domain,
                out=out.data_ptr(), counts=counts.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cdc_eval_auc_delong(a["pred_a"], a["pred_b"], a["label"], a["domain"], 1, a["n"], a["n_domain"], a["out"], a["counts"],
                                       err.data_ptr(), a["ws"], a["ws_bytes"], stream)

    for kw in ({"pred_a": None}, {"label": None}, {"out": None}, {"counts": None}, {"ws": None}, {"domain": None},
               {"n": 0}, {"n": -1}, {"n_domain": 0}, {"n_domain": -2}, {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": ws.data_ptr() + 8}):
        assert call(**kw) == -1, kw                             # CDC_E_BADARG
    assert call(n=1 << 31) == -2 and call(n=1 << 33) == -2      # CDC_E_TOOBIG
    torch.cuda.synchronize()
    assert (out == -3.0).all() and (counts == -3).all() and int(err.item()) == -3 and not ws.any()      # nothing ran
    err.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(counts[n_domain].item()) == n and int(counts[0].item()) == n and int(err.item()) == 0
    res, args = _lib._SIGNATURES["cdc_eval_auc_delong"]
    assert res is C.c_int32 and len(args) == 13 and args[4:7] == [C.c_int64, C.c_int64, C.c_int32] and args[11] is C.c_int64
