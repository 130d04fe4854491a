"""cdc_eval_isotonic_fit / cdc_eval_isotonic_apply / Recalibration / Evaluator(recalibration=...) on the device against the exact
integer fit of tests/isotonic_exact.py (tests/test_isotonic_cpu.py holds that to textbook PAV and to sklearn).

The fit is compared BIT FOR BIT: block bounds are scores that were in the input, counts are integers, and a value is one correctly
rounded division of two integers below 2^31 — there is no tolerance to grant.  The map is compared bit for bit as well: its float64
operations and their order are part of the contract.  The local launch joins spans of 1, 2, .., 1024 points and every merge launch
spans of 1024 * 2^k, all in sorted positions of the 2n keys; the sizes 2^k - 1, 2^k, 2^k + 1 for k = 6..14 put a segment's start and
end on, before and behind every one of those bounds (the "all" segment starts at position n)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from isotonic_exact import isotonic_apply, isotonic_exact

pytestmark = pytest.mark.gpu
FIT_FIELDS = ("start", "x_lo", "x_hi", "count", "positives", "value", "rows", "seg_positives")


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


def _fit(cuda, y, p, dom=None, n_domain=1, strided=False):
    """-> ({field: numpy array, the block fields cut to the number of blocks}, err, the device IsotonicFit)"""
    from cdcmdr_amd.evaluate import eval_isotonic_fit
    n = len(y)
    pred = torch.from_numpy(np.array(p, dtype=np.float32)).to(cuda)
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    f = eval_isotonic_fit(pred, label, _dev_domain(cuda, dom, n, strided), n_domain)
    assert f._fields == FIT_FIELDS
    want = {"start": (torch.int64, n_domain + 2), "rows": (torch.int64, n_domain + 1), "seg_positives": (torch.int64, n_domain + 1),
            "x_lo": (torch.float32, 2 * n), "x_hi": (torch.float32, 2 * n), "count": (torch.int64, 2 * n), "positives": (torch.int64, 2 * n),
            "value": (torch.float64, 2 * n)}
    for k in FIT_FIELDS:
        t = getattr(f, k)
        assert t.is_cuda and t.dtype == want[k][0] and t.shape == (want[k][1],), k
    out = {k: getattr(f, k).cpu().numpy().copy() for k in FIT_FIELDS}
    nb = int(out["start"][-1])
    assert 0 < nb <= 2 * n
    for k in ("x_lo", "x_hi", "count", "positives", "value"):
        out[k] = out[k][:nb]
    return out, int(eval_isotonic_fit.last_err.item()), f


def _expected(fits):
    blocks = [b for f in fits for b in f]
    return {"start": np.cumsum([0] + [len(f) for f in fits]).astype(np.int64),
            "x_lo": np.array([b[0] for b in blocks], np.float32), "x_hi": np.array([b[1] for b in blocks], np.float32),
            "count": np.array([b[2] for b in blocks], np.int64), "positives": np.array([b[3] for b in blocks], np.int64),
            "value": np.array([np.float64(b[3]) / np.float64(b[2]) for b in blocks], np.float64),
            "rows": np.array([sum(b[2] for b in f) for f in fits], np.int64),
            "seg_positives": np.array([sum(b[3] for b in f) for f in fits], np.int64)}


def _bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _check(got, fits, what=""):
    vals, err, _ = got
    assert err == 0, what
    want = _expected(fits)
    for k in FIT_FIELDS:
        assert vals[k].shape == want[k].shape, (what, k, vals[k].shape, want[k].shape, vals["start"], want["start"])
        assert np.array_equal(_bits(vals[k]), _bits(want[k])), (what, k, vals[k], want[k])


def _same_bits(a, b):
    return all(a[0][k].shape == b[0][k].shape and np.array_equal(_bits(a[0][k]), _bits(b[0][k])) for k in FIT_FIELDS)


def _ctr_like(rng, n):
    """most mass below 0.1, and a tie run of a tenth of the rows"""
    p = (rng.random(n) ** 5).astype(np.float32)
    p[rng.random(n) < 0.1] = np.float32(0.03125)
    y = (rng.random(n) < 0.03 + 0.6 * p).astype(np.int16)
    return p, y


def _pattern(name, n):
    if name == "one-block":                                     # every join trims everything: whole chunks empty out
        return (np.arange(n) < n // 2).astype(np.int16)
    if name == "staircase":                                     # runs [1, 0, .., 0] of lengths m, m-1, .., 1: about sqrt(2n) blocks
        m = int((2 * n) ** 0.5) + 2
        return np.concatenate([np.r_[1, np.zeros(k - 1, np.int16)] for k in range(m, 0, -1)])[:n].astype(np.int16)
    if name == "sawtooth":                                      # collinear at every level
        return (np.arange(n) % 2 == 0).astype(np.int16)
    assert name == "late pull-back"                             # the last block reaches back across chunk bounds and stops inside one
    y = (np.random.default_rng(n).random(n) < 0.5).astype(np.int16)
    y[n - n // 8:] = 0
    return y


PATTERNS = ("one-block", "staircase", "sawtooth", "late pull-back")
SIZES = sorted({(1 << k) + o for k in range(6, 15) for o in (-1, 0, 1)})


def test_hand_cases(cuda):
    cases = [([1], [0.25]), ([0], [0.7]),
             ([1, 0], [0.5, 0.5]),                              # two tied rows: one block of 2 with 1 positive
             ([1, 0, 1, 0], [0.1, 0.2, 0.3, 0.4]),              # ONE block of mean 1/2
             ([0, 1, 0, 1], [0.1, 0.2, 0.3, 0.4]),              # 0, 1/2, 1
             ([1, 1, 1], [0.1, 0.2, 0.3]), ([0, 0, 0], [0.3, 0.2, 0.1]),          # one class
             ([0, 1, 1, 0, 1], [0.5] * 5),                      # one score
             ([1, 0, 0, 1], [-0.0, 0.0, -0.0, 0.5]),            # -0.0 beside +0.0
             ([1, 0, 1, 0, 1], [-3.5, -1.0, 0.5, 2.5, 1e30]),   # logits
             ([0, 1, 0, 1, 1], [0.125, 0.25, 0.25, 0.75, 1.0])]                   # INTEGRATION.md's five rows
    for y, p in cases:
        _check(_fit(cuda, y, p), isotonic_exact(y, np.array(p, np.float32)), f"{y}/{p}")
    got = _fit(cuda, [1, 0], [0.5, 0.5])[0]
    assert got["start"].tolist() == [0, 1, 2] and got["count"].tolist() == [2, 2] and got["positives"].tolist() == [1, 1]
    got = _fit(cuda, [1, 0, 1, 0], [0.1, 0.2, 0.3, 0.4])[0]
    assert got["start"].tolist() == [0, 1, 2] and got["value"].tolist() == [0.5, 0.5]
    got = _fit(cuda, [0, 1, 0, 1], [0.1, 0.2, 0.3, 0.4])[0]
    assert got["start"].tolist() == [0, 3, 6] and got["value"].tolist() == [0.0, 0.5, 1.0] * 2
    got = _fit(cuda, [1, 0, 0, 1], [-0.0, 0.0, -0.0, 0.5])[0]
    assert got["x_lo"].tolist() == [0.0, 0.5] * 2 and not np.signbit(got["x_lo"]).any() and got["count"].tolist() == [3, 1] * 2
    got = _fit(cuda, [0, 1, 0, 1, 1], [0.125, 0.25, 0.25, 0.75, 1.0])[0]
    assert got["x_lo"][:3].tolist() == [0.125, 0.25, 0.75] and got["x_hi"][:3].tolist() == [0.125, 0.25, 1.0]
    assert got["value"][:3].tolist() == [0.0, 0.5, 1.0]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_structured_patterns_at_every_span_bound(cuda, pattern):
    for n in SIZES:
        y = _pattern(pattern, n)
        p = np.arange(n, dtype=np.float32)
        _check(_fit(cuda, y, p), isotonic_exact(y, p), f"{pattern}/{n}")


def test_domains_carrying_patterns(cuda):
    rng = np.random.default_rng(11)
    for trial in range(6):
        sizes = [int(s) for s in rng.integers(300, 5000, size=3)]
        names = rng.permutation(PATTERNS)[:3]
        y = np.concatenate([_pattern(nm, s) for nm, s in zip(names, sizes)])
        p = np.concatenate([np.arange(s, dtype=np.float32) * np.float32(0.5) for s in sizes])
        dom = np.concatenate([np.full(s, d, np.int32) for d, s in enumerate(sizes)])
        perm = rng.permutation(len(y))
        y, p, dom = y[perm], p[perm], dom[perm]
        _check(_fit(cuda, y, p, dom, 3, strided=bool(trial % 2)), isotonic_exact(y, p, dom, 3), f"{names}/{sizes}")


def test_empty_and_one_row_domains_and_the_strided_column(cuda):
    rng = np.random.default_rng(9)
    n, n_domain = 900, 6
    p, y = _ctr_like(rng, n)
    dom = rng.choice([0, 2, 3], size=n).astype(np.int32)        # 1 and 5 are empty
    y[dom == 2] = 0
    dom[17] = 4                                                 # one row
    want = isotonic_exact(y, p, dom, n_domain)
    assert want[1] == [] and want[5] == [] and len(want[2]) == 1 and len(want[4]) == 1
    got = _fit(cuda, y, p, dom, n_domain, strided=True)
    _check(got, want, "segments")
    assert got[0]["start"][1] == got[0]["start"][2] and got[0]["rows"].tolist()[1] == 0
    assert _same_bits(got, _fit(cuda, y, p, dom, n_domain))     # the strided column changes nothing


def test_fifty_domains_of_ctr_like_rows(cuda):
    rng = np.random.default_rng(50)
    n, n_domain = 20_000, 50
    p, y = _ctr_like(rng, n)
    dom = rng.choice(n_domain, size=n, p=np.arange(1, n_domain + 1) / (n_domain * (n_domain + 1) / 2)).astype(np.int32)
    _check(_fit(cuda, y, p, dom, n_domain), isotonic_exact(y, p, dom, n_domain), "50 domains")


def test_row_permutations_give_the_same_bits(cuda):
    rng = np.random.default_rng(5)
    n, n_domain = 3000, 2
    p = rng.choice(np.array([0.02, 0.05, 0.05, 0.05, 0.2, 0.6, 0.61], dtype=np.float32), size=n)
    p[::3] = rng.random(len(p[::3])).astype(np.float32)
    y = (rng.random(n) < 0.4).astype(np.int16)
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    got = _fit(cuda, y, p, dom, n_domain)
    _check(got, isotonic_exact(y, p, dom, n_domain), "ties")
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(n)
        assert _same_bits(got, _fit(cuda, y[perm], p[perm], dom[perm], n_domain, strided=True)), seed


@functools.lru_cache(maxsize=None)
def _big():
    n = 70_001
    rng = np.random.default_rng(n)
    p, y = _ctr_like(rng, n)
    p[:4] = [-0.0, 0.0, 1.0, 1e-42]
    dom = rng.choice(3, size=n, p=[0.6, 0.3, 0.1]).astype(np.int32)
    for a in (p, y, dom):
        a.setflags(write=False)
    return y, p, dom


def test_one_large_segment(cuda):
    y, p, _ = _big()
    _check(_fit(cuda, y, p), isotonic_exact(y, p), "70001")


def test_large_three_domains(cuda):
    y, p, dom = _big()
    _check(_fit(cuda, y, p, dom, 3, strided=True), isotonic_exact(y, p, dom, 3), "70001/3")


def _host_apply(fits, seg_of_domain, x, dom, eps):
    out = np.empty(len(x), np.float32)
    for d in np.unique(dom):
        m = dom == d
        out[m] = isotonic_apply(fits[seg_of_domain[d]], x[m], eps)
    return out


def test_apply_matches_the_contract_bit_for_bit(cuda):
    from cdcmdr_amd.evaluate import eval_isotonic_apply
    rng = np.random.default_rng(21)
    n, n_domain = 4000, 3
    p, y = _ctr_like(rng, n)
    p[:300] = rng.normal(0.5, 1.0, 300).astype(np.float32)      # scores below 0 and above 1
    dom = rng.choice(n_domain, size=n, p=[0.7, 0.25, 0.05]).astype(np.int32)
    fits = isotonic_exact(y, p, dom, n_domain)
    _, err, f = _fit(cuda, y, p, dom, n_domain)
    assert err == 0
    knots = np.array([b[k] for s in fits for b in s for k in (0, 1)], np.float32)
    fresh = np.concatenate([p, knots, np.nextafter(knots, np.float32(-np.inf)), np.nextafter(knots, np.float32(np.inf)),
                            (knots[:-1] + knots[1:]) / np.float32(2), rng.uniform(-3, 3, 2000).astype(np.float32),
                            np.array([-1e30, 1e30, -np.inf, np.inf, 0.0, -0.0, 1.0], np.float32)])
    fresh_dom = rng.integers(0, n_domain, size=len(fresh)).astype(np.int32)
    fresh_dom[:n] = dom                                         # the fit rows in their own domains
    xt, dt = torch.from_numpy(fresh).to(cuda), torch.from_numpy(fresh_dom).to(cuda)
    for table in ([0, 1, 2], [0, 3, 3], [3, 3, 3]):             # the identity, fallbacks to "all"
        for eps in (0.0, 1e-6):
            got = eval_isotonic_apply(xt, f, dt, n_domain, None if table == [0, 1, 2] else torch.tensor(table, dtype=torch.int32), eps)
            assert got.is_cuda and got.dtype == torch.float32 and got.shape == (len(fresh),)
            assert int(eval_isotonic_apply.last_err.item()) == 0
            want = _host_apply(fits, table, fresh, fresh_dom, eps)
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (table, eps)
            if eps:
                assert float(got.min()) >= np.float32(1e-6) and float(got.max()) <= np.float32(1) - np.float32(1e-6)
    # monotone in the score within a domain
    got = eval_isotonic_apply(xt, f, dt, n_domain).cpu().numpy()
    for d in range(n_domain):
        m = (fresh_dom == d) & np.isfinite(fresh)
        o = np.argsort(fresh[m], kind="stable")
        assert (np.diff(got[m][o]) >= 0).all(), d
    # a NaN score and a domain outside range: NaN out, the error word names the last such row
    bad_x, bad_d = xt[:8].clone(), dt[:8].clone()
    bad_x[2] = float("nan")
    bad_d[5] = n_domain
    got = eval_isotonic_apply(bad_x, f, bad_d, n_domain).cpu().numpy()
    assert int(eval_isotonic_apply.last_err.item()) == 6 and np.isnan(got).tolist() == [False, False, True, False, False, True, False, False]


def test_recalibrated_fit_rows_are_calibrated(cuda):
    """pcoc and Brier of the recalibrated FIT rows, by eval_calibration.  A block's rows all get float32(value): one rounding,
    relative 2^-24, of a mean whose count-weighted sum is the segment's positives; eval_calibration quantises a prediction to a
    multiple of 2^-32, off by half a unit per row at the most: |pcoc - 1| <= 2^-24 + m / (positives 2^33).  The fit minimises the
    squared error over non-decreasing functions of the score and the identity is one of them (scores in [0, 1]), the roundings move
    a row's squared error by less than 2 * (2^-25 + 2^-33): brier_recal <= brier_raw + 2^-22."""
    from cdcmdr_amd.evaluate import eval_calibration, eval_isotonic_apply
    rng = np.random.default_rng(33)
    n, n_domain = 30_000, 4
    p, y = _ctr_like(rng, n)
    dom = rng.choice(n_domain, size=n, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    p[dom == 1] = np.minimum(np.float32(1), p[dom == 1] * np.float32(3))         # a domain that over-predicts
    pt, yt, dt = torch.from_numpy(p).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(dom).to(cuda)
    _, err, f = _fit(cuda, y, p, dom, n_domain)
    assert err == 0
    recal = eval_isotonic_apply(pt, f, dt, n_domain)
    seg_of_all = torch.full((n_domain,), n_domain, dtype=torch.int32)
    for pred, name in ((recal, "own map"), (eval_isotonic_apply(pt, f, dt, n_domain, seg_of_all), "all")):
        raw, cal = eval_calibration(pt, yt, dt, n_domain), eval_calibration(pred, yt, dt, n_domain)
        assert int(eval_calibration.last_err.item()) == 0
        rows, pos = cal.rows.cpu().tolist(), cal.positives.cpu().tolist()
        pcoc, b1, b0 = cal.pcoc.cpu().tolist(), cal.brier.cpu().tolist(), raw.brier.cpu().tolist()
        for s in (range(n_domain + 1) if name == "own map" else [n_domain]):
            assert 0 < pos[s] < rows[s]
            bound = 2.0 ** -24 + rows[s] / (pos[s] * 2.0 ** 33)
            print(name, s, "pcoc - 1", pcoc[s] - 1, "bound", bound, "brier", b1[s], "raw", b0[s])
            assert abs(pcoc[s] - 1) <= bound, (name, s, pcoc[s], bound)
            assert b1[s] <= b0[s] + 2.0 ** -22, (name, s, b1[s], b0[s])
    assert abs(raw.pcoc.cpu().tolist()[1] - 1) > 0.1            # there was something to repair


def test_bad_rows_set_the_error_word(cuda):
    from cdcmdr_amd.evaluate import Recalibration
    p = np.array([0.2, 0.3, 0.7, 0.6, 0.1, 0.4], dtype=np.float32)
    y = [0, 1, 1, 0, 1, 0]
    good = _fit(cuda, y, p)
    assert good[1] == 0

    def raises(row, y, p, dom=None, n_domain=1):
        with pytest.raises(ValueError, match=f"row {row}:"):
            Recalibration.fit(torch.from_numpy(np.array(p, np.float32)).to(cuda), torch.tensor(y, dtype=torch.int16, device=cuda),
                              None if dom is None else torch.tensor(dom, dtype=torch.int32, device=cuda), n_domain)

    for v in (np.nan, np.inf, -np.inf):
        bad = p.copy()
        bad[3] = v
        got = _fit(cuda, y, bad)
        assert got[1] == 4 and got[0]["rows"].tolist() == [6, 6] and int(got[0]["count"].sum()) == 12      # the launch completes
        raises(3, y, bad)
    assert _fit(cuda, [0, 1, 2, 0, 1, 0], p)[1] == 3            # label 2
    raises(2, [0, 1, 2, 0, 1, 0], p)
    got = _fit(cuda, y, p, dom=[0, 1, 0, 1, 2, 1], n_domain=2)  # domain == n_domain
    assert got[1] == 5 and got[0]["rows"].tolist() == [2, 4, 6]
    raises(4, y, p, [0, 1, 0, 1, 2, 1], 2)
    assert _fit(cuda, y, p, dom=[0, -1, 0, 1, 1, 1], n_domain=2)[1] == 2
    raises(1, y, p, [0, -1, 0, 1, 1, 1], 2)
    assert _same_bits(good, _fit(cuda, y, p))


def test_a_captured_fit_and_apply_replay_to_the_eager_bits(cuda):
    from cdcmdr_amd.evaluate import eval_isotonic_apply, eval_isotonic_fit
    n, n_domain = 5000, 3
    data = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        p, y = _ctr_like(rng, n)
        data.append((p, y, rng.integers(0, n_domain, size=n).astype(np.int32)))
    bufs = [torch.from_numpy(a).to(cuda) for a in data[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator
        eval_isotonic_apply(bufs[0], eval_isotonic_fit(bufs[0], bufs[1], bufs[2], n_domain), bufs[2], n_domain)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f = eval_isotonic_fit(bufs[0], bufs[1], bufs[2], n_domain)
        err = eval_isotonic_fit.last_err
        out = eval_isotonic_apply(bufs[0], f, bufs[2], n_domain, eps=1e-6)
        err_apply = eval_isotonic_apply.last_err
    for p, y, dom in (data[1], data[0]):
        for t, a in zip(bufs, (p, y, dom)):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        assert int(err.item()) == 0 and int(err_apply.item()) == 0
        replayed = {k: getattr(f, k).cpu().numpy().copy() for k in FIT_FIELDS}
        replayed_out = out.cpu().numpy().copy()
        eager, _, ef = _fit(cuda, y, p, dom, n_domain)
        nb = int(eager["start"][-1])
        for k in FIT_FIELDS:
            a = replayed[k][:nb] if k in ("x_lo", "x_hi", "count", "positives", "value") else replayed[k]
            assert np.array_equal(_bits(a), _bits(eager[k])), k
        eager_out = eval_isotonic_apply(torch.from_numpy(p).to(cuda), ef, torch.from_numpy(dom).to(cuda), n_domain, eps=1e-6)
        assert np.array_equal(replayed_out.view(np.int32), eager_out.cpu().numpy().view(np.int32))


def test_abi_bad_arguments_launch_nothing(cuda):
    from cdcmdr_amd import _lib
    lib = _lib.load()
    n, n_domain = 100, 3
    seg = n_domain + 1
    assert lib.cdc_eval_isotonic_max_blocks(n, n_domain) == 2 * n and lib.cdc_eval_isotonic_max_blocks(0, n_domain) == 0
    assert lib.cdc_eval_isotonic_max_blocks(1 << 31, 1) == 0 and lib.cdc_eval_isotonic_fit_workspace_bytes(1 << 31, 1) == 0
    pred = torch.rand(n, device=cuda)
    label = torch.zeros(n, dtype=torch.int16, device=cuda)
    dom = torch.zeros(n, dtype=torch.int32, device=cuda)
    cap = 2 * n
    start = torch.full((seg + 1,), -3, dtype=torch.int64, device=cuda)
    x_lo, x_hi = (torch.full((cap,), -3.0, dtype=torch.float32, device=cuda) for _ in range(2))
    count, positives = (torch.full((cap,), -3, dtype=torch.int64, device=cuda) for _ in range(2))
    value = torch.full((cap,), -3.0, dtype=torch.float64, device=cuda)
    rows, seg_pos = (torch.full((seg,), -3, dtype=torch.int64, device=cuda) for _ in range(2))
    out = torch.full((n,), -3.0, dtype=torch.float32, device=cuda)
    err = torch.full((1,), -3, dtype=torch.int32, device=cuda)
    need = lib.cdc_eval_isotonic_fit_workspace_bytes(n, n_domain)
    assert lib.cdc_eval_isotonic_fit_workspace_bytes(100 * n, n_domain) > need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pred=pred.data_ptr(), label=label.data_ptr(), domain=dom.data_ptr(), n=n, n_domain=n_domain, start=start.data_ptr(),
                x_lo=x_lo.data_ptr(), x_hi=x_hi.data_ptr(), count=count.data_ptr(), positives=positives.data_ptr(), value=value.data_ptr(),
                cap=cap, rows=rows.data_ptr(), seg_pos=seg_pos.data_ptr(), ws=ws.data_ptr(), ws_bytes=need, ld=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cdc_eval_isotonic_fit(a["pred"], a["label"], a["domain"], a["ld"], a["n"], a["n_domain"], a["start"], a["x_lo"], a["x_hi"],
                                         a["count"], a["positives"], a["value"], a["cap"], a["rows"], a["seg_pos"], err.data_ptr(), a["ws"],
                                         a["ws_bytes"], stream)

    for kw in ({"pred": None}, {"label": None}, {"ws": None}, {"domain": None}, {"start": None}, {"x_lo": None}, {"x_hi": None}, {"count": None},
               {"positives": None}, {"value": None}, {"rows": None}, {"seg_pos": None}, {"n": 0}, {"n": -5}, {"n_domain": 0}, {"n_domain": 1 << 20},
               {"ld": -1}, {"cap": cap - 1}, {"cap": 0}, {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": ws.data_ptr() + 8}):
        assert call(**kw) == -1, kw                             # CDC_E_BADARG
    assert call(n=1 << 31, cap=1 << 33) == -2                   # CDC_E_TOOBIG
    seg_of = torch.arange(n_domain, dtype=torch.int32, device=cuda)
    good_apply = dict(pred=pred.data_ptr(), domain=dom.data_ptr(), n=n, n_domain=n_domain, seg_of=seg_of.data_ptr(), start=start.data_ptr(),
                      x_lo=x_lo.data_ptr(), x_hi=x_hi.data_ptr(), value=value.data_ptr(), eps=0.0, out=out.data_ptr())

    def apply(**kw):
        a = dict(good_apply, **kw)
        return lib.cdc_eval_isotonic_apply(a["pred"], a["domain"], 1, a["n"], a["n_domain"], a["seg_of"], a["start"], a["x_lo"], a["x_hi"],
                                           a["value"], a["eps"], a["out"], err.data_ptr(), stream)

    for kw in ({"pred": None}, {"domain": None}, {"seg_of": None}, {"start": None}, {"x_lo": None}, {"x_hi": None}, {"value": None}, {"out": None},
               {"n": 0}, {"n_domain": 0}, {"eps": -1e-3}, {"eps": 0.75}):
        assert apply(**kw) == -1, kw
    assert apply(n=1 << 31) == -2
    torch.cuda.synchronize()
    for t in (start, count, positives, rows, seg_pos):
        assert (t == -3).all()
    for t in (x_lo, x_hi, value, out):
        assert (t == -3.0).all()
    assert int(err.item()) == -3 and not ws.any()               # nothing ran
    err.zero_()
    assert call() == 0 and apply() == 0
    torch.cuda.synchronize()
    assert rows.tolist() == [n, 0, 0, n] and seg_pos.tolist() == [0] * 4 and int(err.item()) == 0
    assert start.tolist() == [0, 1, 1, 1, 2] and count[:2].tolist() == [n, n] and value[:2].tolist() == [0.0, 0.0]
    assert (count[2:] == -3).all() and (value[2:] == -3.0).all() and (x_lo[2:] == -3.0).all()      # nothing at or past start[-1] is written
    assert (out == 0.0).all()


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
    from cdcmdr_amd.evaluate import Evaluator, Recalibration, eval_calibration, eval_metrics
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.1, 3: 0.1}
    kw = dict(mode="multi", domain_idx=3, n_domain=4, domain_cnt_weight=w)
    raw_ev = Evaluator(model, **kw)
    res0 = raw_ev.test(loader)
    assert sorted(res0) == ["domain_auc", "domain_loss", "mean_auc", "mean_loss", "total_auc", "total_loss"]     # recalibration=None: today's keys
    pred, label, dom = raw_ev.predict(loader)
    auc, loss, _, _ = (t.cpu().tolist() for t in eval_metrics(pred, label, dom, 4))
    assert res0["total_auc"] == auc[4] and res0["total_loss"] == loss[4]                                           # and today's values
    assert res0["domain_auc"] == {d: auc[d] for d in (0, 1, 3)} and res0["domain_loss"] == {d: loss[d] for d in (0, 1, 3)}
    assert res0["mean_auc"] == sum(w[d] * auc[d] for d in (0, 1, 3))

    r = raw_ev.fit_recalibration(loader)
    assert isinstance(r, Recalibration) and r.n_domain == 4 and r.fallback_domains == [2]
    assert r.seg_of_domain.cpu().tolist() == [0, 1, 4, 3]
    fits = isotonic_exact(y, pred.cpu().numpy(), X[:, 3], 4)
    nb = sum(len(f) for f in fits)
    assert r.start.cpu().tolist() == np.cumsum([0] + [len(f) for f in fits]).tolist() and r.value.shape == (nb,) and r.x_lo.shape == (nb,)
    for s in (0, 3, "all"):
        b = r.blocks(s)
        f = fits[4 if s == "all" else s]
        assert b.count.tolist() == [x[2] for x in f] and b.positives.tolist() == [x[3] for x in f]
        assert np.array_equal(b.x_lo.view(np.int32), np.array([x[0] for x in f], np.float32).view(np.int32))
    assert len(r.blocks(2).count) == 0
    big = raw_ev.fit_recalibration(loader, min_rows=10 ** 6)
    assert big.fallback_domains == [0, 1, 2, 3] and big.seg_of_domain.cpu().tolist() == [4] * 4

    for eps in (0.0, 1e-4):
        ev = Evaluator(model, recalibration=r, recalibration_eps=eps, calibration=True, **kw)
        res = ev.test(loader)
        rp = r.apply(pred, dom, eps)
        assert np.array_equal(rp.cpu().numpy().view(np.int32), _host_apply(fits, [0, 1, 4, 3], pred.cpu().numpy(), X[:, 3], eps).view(np.int32))
        assert torch.equal(ev.predict(loader)[0], rp)
        auc, loss, _, _ = (t.cpu().tolist() for t in eval_metrics(rp, label, dom, 4))
        cal = eval_calibration(rp, label, dom, 4, 10)
        assert res["total_auc"] == auc[4] and res["total_loss"] == loss[4] and res["domain_auc"] == {d: auc[d] for d in (0, 1, 3)}
        assert res["total_pcoc"] == cal.pcoc.cpu().tolist()[4] and res["domain_brier"] == {d: cal.brier.cpu().tolist()[d] for d in (0, 1, 3)}
        assert abs(res["total_pcoc"] - 1) < 1e-3 + 10 * eps     # fitted and evaluated on the same rows
        table, _, segments = ev.calibration_table(loader)
        assert segments == [0, 1, 2, 3, "all"] and np.array_equal(table.count, cal.table.count.cpu().numpy())

    delta = raw_ev.compare(Evaluator(model, recalibration=r, **kw), loader)
    assert np.isfinite(delta["total_delta"]) and sorted(delta["domain_delta"]) == [0, 1, 3]
    assert all(np.isfinite(v) for v in delta["domain_delta"].values())

    sd = {k: v.cpu() for k, v in r.state_dict().items()}        # as a checkpoint carries it
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    r2 = Recalibration().load_state_dict(sd, device=cuda)
    assert r2.n_domain == 4 and r2.fallback_domains == [2]
    assert torch.equal(r2.apply(pred, dom, 1e-4).view(torch.int32), r.apply(pred, dom, 1e-4).view(torch.int32))

    with pytest.raises(ValueError, match="domain_idx"):
        Evaluator(model, mode="multi", n_domain=4, recalibration=r)

    # mode "single" without a domain column: the one-segment map
    class First(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, X):
            return self.inner(X)[:, :1]

    single = [(Xb, yb) for Xb, yb, _ in loader]
    ev1 = Evaluator(First(model), mode="single")
    r1 = ev1.fit_recalibration(single)
    assert r1.n_domain == 1 and r1.fallback_domains == []
    p1 = ev1.predict(single)[0]
    got = Evaluator(First(model), mode="single", recalibration=r1).predict(single)[0]
    want = isotonic_apply(isotonic_exact(y, p1.cpu().numpy())[0], p1.cpu().numpy())
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
