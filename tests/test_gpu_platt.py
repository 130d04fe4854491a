"""cdc_eval_platt_fit / cdc_eval_platt_apply / PlattRecalibration / Evaluator(recalibration=...) on the device against the float64
restatement of tests/platt_exact.py (tests/test_platt_cpu.py holds that to closed forms and to sklearn).

Acceptance per non-empty segment: CONVERGED is set; the mean gradient recomputed in numpy float64 at the device's (a, b) is <= 1e-9
(10 x gtol: the two math libraries differ by a few ulp on terms of at most Z = 16.1, about 1e-14 per row, and the order of summation
differs — both far below the margin); max |theta_dev - theta_ref| <= 2 |inv(mean Hessian)|_inf 1e-9 (Newton's bound, the factor 2 for
the second-order remainder); the losses inherit that bound times (Z + 1), the largest slope the plain BCE can have in (a, b), plus
1e-12 for the sums themselves; rows and positives are exact.  The pass launch cuts the 2n sorted positions into chunks of 2048 and
the "all" segment starts at position n, so the sizes 2^k - 1, 2^k, 2^k + 1 for k = 6..14 put a segment's start and end on, before
and behind a chunk bound (n = 1023..1025, 2047..2049, ..) and give segments of one piece and of many."""
import functools

import numpy as np
import pytest
import torch

import platt_exact as PX

pytestmark = pytest.mark.gpu
FIELDS = ("a", "b", "rows", "positives", "loss_before", "loss_after", "grad", "iterations", "status")
GTOL = 1e-10


def _dev_domain(cuda, dom, n, strided):
    if dom is None:
        return None
    if strided:                                                 # the domain as a column of an [n, 3] id matrix
        X = np.full((n, 3), -7, dtype=np.int32)
        X[:, 1] = dom
        dt = torch.from_numpy(X).to(cuda)[:, 1]
        assert dt.stride(0) == 3
        return dt
    return torch.from_numpy(np.asarray(dom).astype(np.int32)).to(cuda)


def _fit(cuda, y, p, dom=None, n_domain=1, strided=False, **kw):
    """-> ({field: numpy array}, err, the device PlattFit)"""
    from cdcmdr_amd.evaluate import eval_platt_fit
    n = len(y)
    pred = torch.from_numpy(np.array(p, dtype=np.float32)).to(cuda)
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    f = eval_platt_fit(pred, label, _dev_domain(cuda, dom, n, strided), n_domain, **kw)
    assert f._fields == FIELDS
    want = {"a": torch.float64, "b": torch.float64, "rows": torch.int64, "positives": torch.int64, "loss_before": torch.float64,
            "loss_after": torch.float64, "grad": torch.float64, "iterations": torch.int32, "status": torch.int32}
    for k in FIELDS:
        t = getattr(f, k)
        assert t.is_cuda and t.dtype == want[k] and t.shape == (n_domain + 1,), k
    return {k: getattr(f, k).cpu().numpy().copy() for k in FIELDS}, int(eval_platt_fit.last_err.item()), f


def _bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in FIELDS)


def _accept(got, ref, what="", clip=1e-7, max_iter=32):
    vals, err = got[0], got[1]
    assert err == 0, what
    Z = float(np.log((1 - clip) / clip))
    for s, r in enumerate(ref):
        w = (what, s)
        assert vals["rows"][s] == r["rows"] and vals["positives"][s] == r["positives"], w
        a, b, status = float(vals["a"][s]), float(vals["b"][s]), int(vals["status"][s])
        if r["rows"] == 0:
            assert (a, b, status, int(vals["iterations"][s])) == (1.0, 0.0, PX.EMPTY, 0), w
            assert np.isnan(vals["loss_before"][s]) and np.isnan(vals["loss_after"][s]) and np.isnan(vals["grad"][s]), w
            continue
        assert status == r["status"], (w, status, r["status"])                                 # CONVERGED, and SLOPE_FIXED exactly where the z is one value
        assert 0 <= vals["iterations"][s] <= max_iter and 0 <= vals["grad"][s] <= GTOL, (w, vals["iterations"][s], vals["grad"][s])
        g = PX.mean_gradient(r["z"], r["y"], a, b, r["free"])
        bound = 2.0 * PX.inv_norm(r["H"], r["free"]) * 1e-9
        d = max(abs(a - r["a"]), abs(b - r["b"]))
        print(f"{what} segment {s}: rows {r['rows']} steps {vals['iterations'][s]} mean gradient {g:.2e} |dtheta| {d:.2e} (bound {bound:.2e})")
        assert g <= 1e-9, (w, g)
        assert d <= bound, (w, d, bound)
        for k, other in enumerate(("a", "b")):                                                  # a parameter that is not free has not moved
            if k not in r["free"]:
                assert vals[other][s] == (1.0, 0.0)[k], w
        assert abs(vals["loss_before"][s] - r["loss_before"]) <= 1e-12 * max(1.0, r["loss_before"]), w
        assert abs(vals["loss_after"][s] - r["loss_after"]) <= (Z + 1.0) * bound + 1e-12 * max(1.0, r["loss_after"]), w


@functools.lru_cache(maxsize=None)
def _sized(kind, n):
    return PX.ctr_like(np.random.default_rng(n), n, kind)


@functools.lru_cache(maxsize=None)
def _sized_ref(kind, n, method):
    p, y = _sized(kind, n)
    return PX.platt_exact(y, p, None, 1, method)


SIZES = sorted({(1 << k) + o for k in range(6, 15) for o in (-1, 0, 1)})


def test_hand_cases(cuda):
    # a constant score under "bias" (and under "platt", which holds the slope): b = logit(mean target) - z
    for y, c in [([1, 0, 0, 0], 0.3), ([0, 0, 0], 0.9), ([1], 0.01), ([1, 1, 0, 1, 0, 0, 0, 1, 1], 0.5)]:
        p = np.full(len(y), c, np.float32)
        z = PX.platt_z(p)[0]
        t = np.mean(PX.targets(y))
        for method in ("bias", "platt"):
            got = _fit(cuda, y, p, method=method)
            _accept(got, PX.platt_exact(y, p, None, 1, method), f"constant {c} {method}")
            assert got[0]["a"].tolist() == [1.0, 1.0] and np.abs(got[0]["b"] - (np.log(t) - np.log1p(-t) - z)).max() <= 2e-9 / (t * (1 - t)) + 1e-12
            assert got[0]["status"].tolist() == [PX.CONVERGED | (PX.SLOPE_FIXED if method == "platt" else 0)] * 2
    # two distinct scores under "platt": the map reproduces each group's mean target
    y = np.array([1, 0, 0, 0, 0, 1, 1, 0, 1, 0])
    p = np.array([0.1] * 5 + [0.6] * 5, np.float32)
    got = _fit(cuda, y, p)
    _accept(got, PX.platt_exact(y, p), "two scores")
    z, t = PX.platt_z(p), PX.targets(y)
    for k in (0, 5):
        assert abs(PX.sigmoid(got[0]["a"][0] * z[k] + got[0]["b"][0]) - np.mean(t[k:k + 5])) <= 1e-9
    # temperature where every z is 0: converged at the start, no step
    got = _fit(cuda, [1, 0, 0, 1], [0.5] * 4, method="temperature")
    assert got[0]["a"].tolist() == [1.0, 1.0] and got[0]["iterations"].tolist() == [0, 0] and got[0]["status"].tolist() == [PX.CONVERGED] * 2
    # one class, separable rows, both ends of the clamp, one row
    for y, p in [([0, 0, 0], [0.2, 0.4, 0.7]), ([1, 1], [0.2, 0.4]), ([0, 0, 1, 1], [0.1, 0.2, 0.8, 0.9]), ([0, 1, 1, 1, 0], [0.0, 1.0, 0.0, 1.0, 0.5]),
                 ([1], [0.25]), ([0], [0.0])]:
        for method in PX.METHODS:
            _accept(_fit(cuda, y, p, method=method), PX.platt_exact(y, np.array(p, np.float32), None, 1, method), f"{y}/{p} {method}")
    # INTEGRATION.md's five rows
    p, y = np.array([0.125, 0.25, 0.25, 0.75, 0.875], np.float32), [0, 1, 0, 1, 1]
    for method, a, b, loss in (("bias", 1.0, 0.797094070225849, 0.37732765846475746), ("platt", 0.6068824258608988, 0.5402678889181521, 0.4479523301497436),
                               ("temperature", 0.51065698033196, 0.0, 0.5090737141590544)):
        got = _fit(cuda, y, p, method=method)
        _accept(got, PX.platt_exact(y, p, None, 1, method), f"five rows {method}")
        assert abs(got[0]["a"][1] - a) < 5e-7 and abs(got[0]["b"][1] - b) < 5e-7 and abs(got[0]["loss_after"][1] - loss) < 5e-7      # as printed there
        assert abs(got[0]["loss_before"][0] - 0.4457442582544996) < 5e-7
        if method != "temperature":
            assert abs(PX.platt_apply(p, got[0]["a"][0], got[0]["b"][0]).astype(np.float64).sum() - 2.9) < 1e-6
    # another clip
    p, y = _sized("odds x10", 257)
    _accept(_fit(cuda, y, p, clip=0.01), PX.platt_exact(y, p, clip=0.01), "clip 0.01", clip=0.01)


@pytest.mark.parametrize("method", PX.METHODS)
@pytest.mark.parametrize("kind", PX.KINDS)
def test_one_segment_at_every_chunk_bound(cuda, kind, method):
    steps = 0
    for n in SIZES:
        p, y = _sized(kind, n)
        got = _fit(cuda, y, p, method=method)
        _accept(got, _sized_ref(kind, n, method), f"{kind}/{method}/{n}")
        steps = max(steps, int(got[0]["iterations"].max()))
    print(f"{kind}/{method}: at most {steps} Newton steps on the device, {PX.STATS['steps']} in the reference")


def _skewed(n_domain, n=5000, seed=5):
    """skewed domain sizes; domain 1 is empty, domain 2 has one row (one class, one score); past three domains the last one has a
    single class and domain 3 a constant score"""
    rng = np.random.default_rng(seed)
    p, y = PX.ctr_like(rng, n, "slope 0.4 shift -1")
    w = 1.0 / (1.0 + np.arange(n_domain)) ** 1.2
    w[[1, 2]] = 0.0
    if n_domain > 3:
        w[n_domain - 1] = max(w[n_domain - 1], 0.02)
    dom = rng.choice(n_domain, size=n, p=w / w.sum())
    dom[0] = 2
    if n_domain > 3:
        y[dom == n_domain - 1] = 0
        p[dom == 3] = np.float32(0.0625)
    return p, y, dom.astype(np.int32)


@pytest.mark.parametrize("n_domain", [3, 50])
def test_skewed_domains(cuda, n_domain):
    p, y, dom = _skewed(n_domain)
    for method in PX.METHODS:
        ref = PX.platt_exact(y, p, dom, n_domain, method)
        got = _fit(cuda, y, p, dom, n_domain, method=method)
        _accept(got, ref, f"{n_domain} domains/{method}")
        status = got[0]["status"]
        assert [s for s in range(n_domain + 1) if status[s] & PX.EMPTY] == [1]
        fixed = [2] + ([3] if n_domain > 3 else [])
        assert [s for s in range(n_domain + 1) if status[s] & PX.SLOPE_FIXED] == (fixed if method == "platt" else [])
        assert got[0]["rows"][2] == 1 and (n_domain == 3 or (got[0]["positives"][n_domain - 1] == 0 and got[0]["rows"][n_domain - 1] > 1))
        one = _fit(cuda, y, p, method=method)[0]                # the "all" segment lies at the same sorted positions: the same bits
        for k in FIELDS:
            assert _bits(got[0][k])[n_domain] == _bits(one[k])[1], (method, k)


def test_row_permutations_and_the_strided_column_give_the_same_bits(cuda):
    for n_domain, n in ((3, 5000), (50, 5000), (1, 4097)):
        p, y, dom = _skewed(n_domain, n) if n_domain > 1 else (*_sized("odds x10", n), np.zeros(n, np.int32))
        for method in PX.METHODS:
            base = _fit(cuda, y, p, dom, n_domain, method=method)[0]
            for seed in (1, 2):
                perm = np.random.default_rng(seed).permutation(n)
                other = _fit(cuda, y[perm], p[perm], dom[perm], n_domain, strided=seed == 2, method=method)[0]
                assert _same_bits(base, other), (n_domain, method, seed)


def test_logit_input(cuda):
    rng = np.random.default_rng(11)
    x, y = PX.ctr_like(rng, 3000, "slope 0.4 shift -1", input="logit")
    x[:8] = np.array([np.inf, -np.inf, 1e30, -1e30, np.inf, -1e30, 40.0, -40.0], np.float32)
    y[:8] = [1, 0, 1, 0, 0, 1, 1, 0]
    for method in PX.METHODS:
        _accept(_fit(cuda, y, x, method=method, input="logit"), PX.platt_exact(y, x, None, 1, method, "logit"), f"logit/{method}")
    a = _fit(cuda, y, x, input="logit", clip=1e-3)
    _accept(a, PX.platt_exact(y, x, input="logit", clip=1e-3), "logit/clip 1e-3", clip=1e-3)
    xc = np.clip(x, -np.float32(60), np.float32(60))            # everything past Z is one z (the rows that tie change their order)
    _accept(_fit(cuda, y, xc, input="logit", clip=1e-3), PX.platt_exact(y, x, input="logit", clip=1e-3), "logit/clipped", clip=1e-3)


def test_bad_rows_set_the_error_word(cuda):
    rng = np.random.default_rng(13)
    n = 700
    p, y = PX.ctr_like(rng, n, "calibrated")
    dom = rng.integers(0, 3, size=n).astype(np.int32)
    for row, what in [(5, "nan"), (699, "label"), (300, "domain"), (41, "above"), (42, "below")]:
        p2, y2, d2 = p.copy(), y.copy(), dom.copy()
        if what == "nan":
            p2[row] = np.nan
        elif what == "label":
            y2[row] = 2
        elif what == "domain":
            d2[row] = 3
        else:
            p2[row] = np.float32(1.5 if what == "above" else -0.25)
        got = _fit(cuda, y2, p2, d2, 3)
        assert got[1] == row + 1, what
        p2[row], y2[row], d2[row] = 0.5, 0, min(d2[row], 2)     # counted with z = 0, label 0, the domain clamped
        want = _fit(cuda, y2, p2, d2, 3)
        assert want[1] == 0 and _same_bits(got[0], want[0]), what
    x = p.copy()
    x[[3, 9]] = np.nan
    x[4] = 7.0                                                  # a logit may be anything but NaN
    assert _fit(cuda, y, x, dom, 3, input="logit")[1] == 10
    from cdcmdr_amd.evaluate import PlattRecalibration
    with pytest.raises(ValueError, match="row 9"):
        PlattRecalibration.fit(torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(dom).to(cuda), 3, input="logit")


def _ulps(a, b):
    """distance in float32 steps between two arrays of finite non-negative floats"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_apply(cuda):
    from cdcmdr_amd.evaluate import eval_platt_apply
    rng = np.random.default_rng(17)
    n, n_domain = 5000, 4
    p, y = PX.ctr_like(rng, n, "odds x10")
    p[:4] = [0.0, 1.0, 0.5, 1e-30]
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    dom[dom == 1] = 0                                           # domain 1 is empty: its rows at apply time go through "all"
    vals, err, f = _fit(cuda, y, p, dom, n_domain)
    assert err == 0
    q, _ = PX.ctr_like(rng, n, "odds x10")
    qd = rng.integers(0, n_domain, size=n).astype(np.int32)
    pt, qt = torch.from_numpy(q).to(cuda), torch.from_numpy(qd).to(cuda)
    for table in (None, [0, 4, 2, 4]):
        for eps in (0.0, 1e-3):
            for strided in (False, True):
                out = eval_platt_apply(pt, f, _dev_domain(cuda, qd, n, strided), n_domain, seg_of_domain=table, eps=eps).cpu().numpy()
                assert int(eval_platt_apply.last_err.item()) == 0
                seg = qd if table is None else np.array(table)[qd]
                want = PX.platt_apply(q, vals["a"][seg], vals["b"][seg], eps=eps)
                assert out.dtype == np.float32 and _ulps(out, want).max() <= 1, (table, eps, _ulps(out, want).max())
                if eps:
                    assert out.min() >= np.float32(eps) and out.max() <= np.float32(1) - np.float32(eps)
    Fit = type(f)                                               # the clamp where the map saturates
    steep = Fit(*(torch.tensor([40.0, 40.0], dtype=torch.float64, device=cuda) if k == "a" else getattr(f, k)[:2] for k in FIELDS))
    assert eval_platt_apply(torch.tensor([0.0, 1.0], device=cuda), steep, None, 1, eps=0.25).cpu().tolist() == [0.25, 0.75]
    # logits
    x = np.array([np.inf, -np.inf, 0.0, 3.5, -2.25], np.float32)
    out = eval_platt_apply(torch.from_numpy(x).to(cuda), steep._replace(a=torch.tensor([0.5, 1.0], dtype=torch.float64, device=cuda),
                                                                        b=torch.tensor([-1.0, 0.0], dtype=torch.float64, device=cuda)),
                           None, 1, input="logit").cpu().numpy()
    assert _ulps(out, PX.platt_apply(x, 0.5, -1.0, "logit")).max() <= 1
    # a NaN, a probability outside [0, 1] and a domain outside range give NaN and the error word
    q2, d2 = q.copy(), qd.copy()
    q2[7], q2[100], d2[2000], d2[4999] = np.nan, 1.25, n_domain, -1
    out = eval_platt_apply(torch.from_numpy(q2).to(cuda), f, torch.from_numpy(d2).to(cuda), n_domain).cpu().numpy()
    assert int(eval_platt_apply.last_err.item()) == 5000
    bad = np.zeros(n, bool)
    bad[[7, 100, 2000, 4999]] = True
    assert np.isnan(out[bad]).all() and not np.isnan(out[~bad]).any()
    assert _ulps(out[~bad], PX.platt_apply(q, vals["a"][qd], vals["b"][qd])[~bad]).max() <= 1


def test_recalibration_fallbacks_and_state_dict(cuda):
    from cdcmdr_amd.evaluate import PlattRecalibration
    rng = np.random.default_rng(19)
    n, n_domain = 6000, 6
    p, y = PX.ctr_like(rng, n, "odds x10")
    dom = rng.choice([0, 2, 3, 4, 5], size=n, p=[0.6, 0.01, 0.13, 0.13, 0.13]).astype(np.int32)     # 1: no rows; 2: about 60 rows
    y[dom == 3] = 0                                                                                  # 3: one class
    anti = dom == 4                                                                                  # 4: the higher the score, the fewer positives
    y[anti] = (rng.random(int(anti.sum())) < 1.0 - np.clip(4 * p[anti], 0, 1)).astype(np.int16)
    t = [torch.from_numpy(a).to(cuda) for a in (p, y, dom)]
    ref = PX.platt_exact(y, p, dom, n_domain)
    assert ref[4]["a"] < 0 < ref[5]["a"] and 0 < ref[2]["rows"] < 200 and ref[2]["a"] > 0
    r = PlattRecalibration.fit(*t, n_domain, min_rows=200)
    assert r.fallback_domains == [1, 2, 3, 4] and r.seg_of_domain.cpu().tolist() == [0, 6, 6, 6, 6, 5]
    assert (r.n_domain, r.method, r.input, r.clip) == (6, "platt", "prob", 1e-7)
    assert PlattRecalibration.fit(*t, n_domain).fallback_domains == [1, 3, 4]
    assert PlattRecalibration.fit(*t, n_domain, need_increasing=False).fallback_domains == [1, 3]
    assert PlattRecalibration.fit(*t, n_domain, need_both_classes=False, need_increasing=False).fallback_domains == [1]
    assert PlattRecalibration.fit(*t, n_domain, method="bias").fallback_domains == [1, 3]                 # a = 1 is increasing
    assert PlattRecalibration.fit(*t, n_domain, method="bias", need_both_classes=False).fallback_domains == [1]
    slow = PlattRecalibration.fit(*t, n_domain, method="bias", max_iter=1)                           # one step does not reach 1e-10 from odds x10
    assert slow.fallback_domains == [0, 1, 2, 3, 4, 5] and not slow.params("all")[2] & PX.CONVERGED
    a, b, status = r.params(5)
    assert status == PX.CONVERGED and max(abs(a - ref[5]["a"]), abs(b - ref[5]["b"])) <= 2 * PX.inv_norm(ref[5]["H"], (0, 1)) * 1e-9
    assert r.params("all") == r.params(6) and r.params(1) == (1.0, 0.0, PX.EMPTY)
    with pytest.raises(ValueError):
        r.params(7)
    out = r.apply(t[0], t[2], 1e-4).cpu().numpy()
    seg = np.array([0, 6, 6, 6, 6, 5])[dom]
    assert _ulps(out, PX.platt_apply(p, r.a.cpu().numpy()[seg], r.b.cpu().numpy()[seg], eps=1e-4)).max() <= 1
    sd = {k: v.cpu() for k, v in r.state_dict().items()}        # as a checkpoint carries it
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    r2 = PlattRecalibration().load_state_dict(sd, device=cuda)
    assert (r2.n_domain, r2.method, r2.input, r2.clip, r2.fallback_domains) == (6, "platt", "prob", 1e-7, [1, 2, 3, 4])
    assert torch.equal(r2.apply(t[0], t[2], 1e-4).view(torch.int32), r.apply(t[0], t[2], 1e-4).view(torch.int32))
    lg = PlattRecalibration.fit(torch.from_numpy(PX.platt_z(p).astype(np.float32)).to(cuda), t[1], t[2], n_domain, input="logit", clip=1e-3)
    lg2 = PlattRecalibration().load_state_dict(lg.state_dict())
    assert (lg2.input, lg2.clip, lg2.method) == ("logit", 1e-3, "platt")


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


def test_evaluator_recalibration(cuda):
    from cdcmdr_amd.evaluate import Evaluator, PlattRecalibration, Recalibration, eval_calibration, eval_metrics
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.1, 3: 0.1}
    kw = dict(mode="multi", domain_idx=3, n_domain=4, domain_cnt_weight=w)
    raw_ev = Evaluator(model, **kw)
    pred, label, dom = raw_ev.predict(loader)
    assert isinstance(raw_ev.fit_recalibration(loader), Recalibration)                               # the default stays what it is
    with pytest.raises(ValueError, match="method"):
        raw_ev.fit_recalibration(loader, method="beta")
    P = {s: int(y[X[:, 3] == s].sum()) if s < 4 else int(y.sum()) for s in (0, 1, 3, 4)}
    M = {s: int((X[:, 3] == s).sum()) if s < 4 else len(y) for s in (0, 1, 3, 4)}

    def smoothed_pcoc(s):                                       # the zero gradient in b: the predictions of a segment sum to its targets
        return (P[s] * (P[s] + 1.0) / (P[s] + 2.0) + (M[s] - P[s]) / (M[s] - P[s] + 2.0)) / P[s]

    for method in ("platt", "temperature", "bias"):
        r = raw_ev.fit_recalibration(loader, method=method, need_increasing=False)
        assert isinstance(r, PlattRecalibration) and r.method == method and r.n_domain == 4 and r.fallback_domains == [2]
        assert r.seg_of_domain.cpu().tolist() == [0, 1, 4, 3]
        ref = PX.platt_exact(y, pred.cpu().numpy(), X[:, 3], 4, method)
        for s in (0, 1, 3, "all"):
            a, b, status = r.params(s)
            q = ref[4 if s == "all" else s]
            assert status == q["status"] and max(abs(a - q["a"]), abs(b - q["b"])) <= 2 * PX.inv_norm(q["H"], q["free"]) * 1e-9
        for eps in (0.0, 1e-4):
            ev = Evaluator(model, recalibration=r, recalibration_eps=eps, calibration=True, **kw)
            res = ev.test(loader)
            rp = r.apply(pred, dom, eps)
            assert torch.equal(ev.predict(loader)[0], rp)
            auc, loss, _, _ = (t.cpu().tolist() for t in eval_metrics(rp, label, dom, 4))
            cal = eval_calibration(rp, label, dom, 4, 10)
            assert res["total_auc"] == auc[4] and res["total_loss"] == loss[4] and res["domain_auc"] == {d: auc[d] for d in (0, 1, 3)}
            assert res["domain_loss"] == {d: loss[d] for d in (0, 1, 3)}
            assert res["total_pcoc"] == cal.pcoc.cpu().tolist()[4] and res["domain_brier"] == {d: cal.brier.cpu().tolist()[d] for d in (0, 1, 3)}
            if method != "temperature" and eps == 0.0:
                for d in (0, 1, 3):
                    assert abs(res["domain_pcoc"][d] - smoothed_pcoc(d)) <= 1e-6, (method, d)
    delta = raw_ev.compare(Evaluator(model, recalibration=r, **kw), loader)
    assert np.isfinite(delta["total_delta"]) and sorted(delta["domain_delta"]) == [0, 1, 3]
    with pytest.raises(ValueError, match="domain_idx"):
        Evaluator(model, mode="multi", n_domain=4, recalibration=r)

    # mode "single" without a domain column: the one-segment map, and total_pcoc of a fit on the evaluated split
    class First(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, X):
            return self.inner(X)[:, :1]

    single = [(Xb, yb) for Xb, yb, _ in loader]
    ev1 = Evaluator(First(model), mode="single")
    p1 = ev1.predict(single)[0]
    for method in ("bias", "platt"):
        r1 = ev1.fit_recalibration(single, method=method, need_increasing=False)     # random labels: the slope may come out negative
        assert r1.n_domain == 1 and r1.fallback_domains == []
        res = Evaluator(First(model), mode="single", recalibration=r1, calibration=True).test(single)
        assert abs(res["total_pcoc"] - smoothed_pcoc(4)) <= 1e-6, method
        got = Evaluator(First(model), mode="single", recalibration=r1).predict(single)[0]
        a, b, _ = r1.params(0)
        assert _ulps(got.cpu().numpy(), PX.platt_apply(p1.cpu().numpy(), a, b)).max() <= 1


def test_a_captured_fit_and_apply_replay_to_the_eager_bits(cuda):
    from cdcmdr_amd.evaluate import eval_platt_apply, eval_platt_fit
    n, n_domain = 5000, 3
    data = [_skewed(n_domain, n, seed) for seed in (1, 2)]
    bufs = [torch.from_numpy(a).to(cuda) for a in data[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator
        eval_platt_apply(bufs[0], eval_platt_fit(bufs[0], bufs[1], bufs[2], n_domain), bufs[2], n_domain)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f = eval_platt_fit(bufs[0], bufs[1], bufs[2], n_domain)
        err = eval_platt_fit.last_err
        out = eval_platt_apply(bufs[0], f, bufs[2], n_domain, eps=1e-6)
    for p, y, dom in (data[1], data[0]):
        for t, a in zip(bufs, (p, y, dom)):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        replayed = {k: getattr(f, k).cpu().numpy().copy() for k in FIELDS}
        replayed_out = out.cpu().numpy().copy()
        eager, _, ef = _fit(cuda, y, p, dom, n_domain)
        assert _same_bits(replayed, eager)
        eager_out = eval_platt_apply(torch.from_numpy(p).to(cuda), ef, torch.from_numpy(dom).to(cuda), n_domain, eps=1e-6)
        assert np.array_equal(replayed_out.view(np.int32), eager_out.cpu().numpy().view(np.int32))
