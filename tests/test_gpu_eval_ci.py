"""cdc_eval_loss_ci / cdc_eval_gauc_ci, eval_loss_ci / eval_gauc_ci and Evaluator(loss_ci=True, gauc_ci=True) on the device against
tests/loss_ci_exact.py (float64, math.log, math.fsum) and tests/gauc_ci_exact.py (exact rationals; tests/test_eval_ci_cpu.py holds
its two forms to each other).  Counts must be equal, NaN must stand exactly where the helper has None, `loss` and `gauc` must be
`eval_metrics`' and `eval_gauc`'s bits.  The bounds are derived, not measured; u = 2^-53.

GAUC (K = the groups counted in the segment; every A_g, B_g, G lies in [0, 1]):
  gauc, gauc_b  tests/test_gpu_gauc.py's bound: (2 K + 8) u |G|.
  delta         G_a - G_b of two such figures and one subtraction: (2 K + 9) u (|G_a| + |G_b|).
  var           the device forms A_g with one rounding (u |A|), reads G with its (2 K + 8) u |G| and subtracts (u |A - G|): the centred
                value c = A - G carries e <= (2 K + 8) u (|A| + |G|) + u |c|.  t = w c and t^2 round once each, so
                |t^2 - exact| <= w^2 (2 |c| e + e^2) + 3 u t^2 <= (4 K + 16) u w^2 |c| (|A| + |G|) + w^2 e^2 + 5 u t^2.  The K terms are
                >= 0 and are added in SOME order ((K - 1) u), sum w likewise and is squared (2 (K - 1) u + u), K / (K - 1) rounds
                once, the product and the quotient once each, the expected value once more (u / 2): (3 K + 6.5) u in all.  With
                abs = K / (K - 1) sum w^2 |A - G| (|A| + |G|) / (sum w)^2 from the helper, and w^2 e^2 summed and scaled
                <= 2 * 4 * ((2 K + 9) u)^2 because |A| + |G| <= 2, sum w^2 <= (sum w)^2 and K / (K - 1) <= 2:
                    |got - want| <= (4 K + 16) u abs + (3 K + 8) u want + 8 ((2 K + 9) u)^2.
  var_delta     the same with c = (A - B) - delta: A - B carries u (|A| + |B|) + u |A - B|, delta its bound above, so
                e <= (2 K + 9) u (|A| + |B| + |G_a| + |G_b|) + u |c|, the bracket <= 4:
                    |got - want| <= (4 K + 18) u abs_delta + (3 K + 8) u want + 32 ((2 K + 9) u)^2.

Log-loss (m = the segment's rows, D = ceil(m / 1024) + 10 = the additions on the longest path of the 1024 strided partial sums
and their tree):
  loss          the 1e-11 relative bound tests/test_gpu_eval.py holds eval_metrics' loss to; delta: 1e-11 (|loss| + |loss_b|).
  var           a term l_i differs from the helper's by two 1-ulp logarithms: d_i = 2^-51 l_i.  The means differ by
                E = mean(d_i) + (D + 3) u mean(|l_i|) (D additions and a division on the device, fsum's one rounding and a division
                in the helper).  The centred value c_i = l_i - mean carries d_i + E + u |c_i|, its square
                2 |c_i| (d_i + E) + (d_i + E)^2 + 3 u c_i^2; the sum adds D u, m (m - 1) and the quotient 2 u on either side:
                    |got - want| <= [sum 2 |c_i| (d_i + E) + sum (d_i + E)^2] / (m (m - 1)) + (D + 12) u want.
  var_delta     the same on t_i = l_i(a) - l_i(b) with d_i = 2^-51 (l_i(a) + l_i(b)) + 2 u |t_i| (four logarithms and the subtraction
                on either side) and mean(|t_i|) in E.
  Another row order changes the order of the additions, nothing else: the same bounds hold, not the same bits."""
import functools
import math

import numpy as np
import pytest
import torch

from gauc_ci_exact import gauc_ci_exact
from loss_ci_exact import as_float, loss_ci_exact

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LOSS_KEYS = ("loss", "var", "loss_b", "var_b", "delta", "var_delta")
GAUC_KEYS = ("gauc", "var", "gauc_b", "var_b", "delta", "var_delta")


def _columns(cuda, n, cols, strided):
    """id columns -> device tensors, contiguous or as strided views of one [n, 4] matrix"""
    if not strided:
        return [None if c is None else torch.from_numpy(np.asarray(c).astype(np.int32)).to(cuda) for c in cols]
    X = np.full((n, 4), -7, dtype=np.int32)
    for k, c in enumerate(cols):
        if c is not None:
            X[:, k + 1] = c
    Xd = torch.from_numpy(X).to(cuda)
    out = [None if c is None else Xd[:, k + 1] for k, c in enumerate(cols)]
    assert all(t is None or t.stride(0) == 4 for t in out)
    return out


def _f32(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(cuda)


def _loss_device(cuda, y, s, sb=None, dom=None, n_domain=1, strided=False):
    """-> ({field: float64 [n_domain + 1]}, rows, positives, err)"""
    from cdcmdr_amd.evaluate import eval_loss_ci
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    dt, = _columns(cuda, len(y), [dom], strided)
    r = eval_loss_ci(_f32(cuda, s), label, dt, n_domain, pred_b=_f32(cuda, sb))
    keys = LOSS_KEYS if sb is not None else LOSS_KEYS[:2]
    assert r._fields == ("loss", "var", "rows", "positives") + keys[2:]
    for t in r:
        assert t.is_cuda and t.numel() == n_domain + 1
    assert r.loss.dtype == r.var.dtype == torch.float64 and r.rows.dtype == r.positives.dtype == torch.int64
    err = int(eval_loss_ci.last_err.item())
    return {k: getattr(r, k).cpu().numpy().copy() for k in keys}, r.rows.cpu().numpy().copy(), r.positives.cpu().numpy().copy(), err


def _gauc_device(cuda, y, s, u, n_user, sb=None, dom=None, n_domain=1, w=None, strided=False):
    """-> ({field: float64 [n_domain + 1]}, counted, left_out, err)"""
    from cdcmdr_amd.evaluate import eval_gauc_ci
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    ut, dt = _columns(cuda, len(y), [u, dom], strided)
    wt = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).to(cuda)
    r = eval_gauc_ci(_f32(cuda, s), label, ut, n_user, dt, n_domain, wt, pred_b=_f32(cuda, sb))
    keys = GAUC_KEYS if sb is not None else GAUC_KEYS[:2]
    assert r._fields == ("gauc", "var", "counted", "left_out") + keys[2:]
    for t in r:
        assert t.is_cuda and t.numel() == n_domain + 1
    assert r.gauc.dtype == r.var.dtype == torch.float64 and r.counted.dtype == r.left_out.dtype == torch.int64
    err = int(eval_gauc_ci.last_err.item())
    return {k: getattr(r, k).cpu().numpy().copy() for k in keys}, r.counted.cpu().numpy().copy(), r.left_out.cpu().numpy().copy(), err


def _var_bound(t, d):
    """the module docstring's bound on a variance of the mean of the values t whose device and helper forms differ by at most d"""
    m = len(t)
    D = -(-m // 1024) + 10
    mean = math.fsum(t) / m
    E = math.fsum(d) / m + (D + 3) * U * math.fsum(abs(v) for v in t) / m
    c = [v - mean for v in t]
    want = math.fsum(v * v for v in c) / (m * (m - 1))
    return (math.fsum(2 * abs(v) * (e + E) for v, e in zip(c, d)) + math.fsum((e + E) ** 2 for e in d)) / (m * (m - 1)) + (D + 12) * U * want


def _loss_bounds(w):
    """{field: bound} of one segment's dict of loss_ci_exact"""
    la = w["terms"]
    b = {"loss": 1e-11 * abs(w["loss"]), "var": _var_bound(la, [2.0 ** -51 * v for v in la])}
    if "terms_b" in w:
        lb = w["terms_b"]
        t = [x - z for x, z in zip(la, lb)]
        b.update({"loss_b": 1e-11 * abs(w["loss_b"]), "var_b": _var_bound(lb, [2.0 ** -51 * v for v in lb]),
                  "delta": 1e-11 * (abs(w["loss"]) + abs(w["loss_b"])),
                  "var_delta": _var_bound(t, [2.0 ** -51 * (x + z) + 2 * U * abs(v) for x, z, v in zip(la, lb, t)])})
    return b


def _check_loss(got, want, what="", err=0):
    vals, rows, pos, got_err = got
    assert got_err == err, (what, got_err, err)
    assert rows.tolist() == [w["rows"] for w in want] and pos.tolist() == [w["P"] for w in want], (what, rows, pos)
    for d, w in enumerate(want):
        bounds = _loss_bounds(w) if w["loss"] is not None else {}
        for k, arr in vals.items():
            print(what, k, d, "device", arr[d], "helper", as_float(w[k]), "bound", bounds.get(k))
            if w[k] is None:
                assert np.isnan(arr[d]), (what, k, d, arr[d])
                continue
            assert abs(arr[d] - w[k]) <= bounds[k], (what, k, d, arr[d], w[k], abs(arr[d] - w[k]), bounds[k])


def _gauc_bounds(w):
    K = w["counted"]
    G = abs(float(w["gauc"]))
    b = {"gauc": (2 * K + 8) * U * G}
    if K >= 2:
        b["var"] = (4 * K + 16) * U * w["abs"] + (3 * K + 8) * U * float(w["var"]) + 8 * ((2 * K + 9) * U) ** 2
    if "gauc_b" in w:
        Gb = abs(float(w["gauc_b"]))
        b.update({"gauc_b": (2 * K + 8) * U * Gb, "delta": (2 * K + 9) * U * (G + Gb)})
        if K >= 2:
            b["var_b"] = (4 * K + 16) * U * w["abs_b"] + (3 * K + 8) * U * float(w["var_b"]) + 8 * ((2 * K + 9) * U) ** 2
            b["var_delta"] = (4 * K + 18) * U * w["abs_delta"] + (3 * K + 8) * U * float(w["var_delta"]) + 32 * ((2 * K + 9) * U) ** 2
    return b


def _check_gauc(got, want, what="", err=0):
    vals, counted, left, got_err = got
    assert got_err == err, (what, got_err, err)
    assert counted.tolist() == [w["counted"] for w in want] and left.tolist() == [w["left_out"] for w in want], (what, counted, left)
    for d, w in enumerate(want):
        bounds = _gauc_bounds(w) if w["gauc"] is not None else {}
        for k, arr in vals.items():
            print(what, k, d, "device", arr[d], "exact", as_float(w[k]), "bound", bounds.get(k))
            if w[k] is None:
                assert np.isnan(arr[d]), (what, k, d, arr[d])
                continue
            assert abs(arr[d] - float(w[k])) <= bounds[k], (what, k, d, arr[d], float(w[k]), abs(arr[d] - float(w[k])), bounds[k])


def _bits(a, b, keys=None):
    return all(np.array_equal(a[0][k].view(np.int64), b[0][k].view(np.int64)) for k in (keys or a[0])) and \
        np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _scores(kind, n, rng):
    if kind == "five":
        return rng.choice(np.array([0.1, 0.25, 0.5, 0.75, 0.9], dtype=np.float32), size=n)        # long tie runs
    if kind == "distinct":
        return rng.permutation(n).astype(np.float32) / np.float32(n + 1)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, 0.5, -0.5], dtype=np.float32)     # signed zeros, denormals
    return rng.choice(pool, size=n)


def _loss_err(*vectors):
    """the error word eval_loss_ci owes: 1 + the last row with a prediction outside [0, 1] (-0.0 is inside)"""
    bad = np.zeros(len(vectors[0]), dtype=bool)
    for v in vectors:
        bad |= ~((v >= 0) & (v <= 1))
    return int(np.flatnonzero(bad)[-1]) + 1 if bad.any() else 0


@pytest.mark.parametrize("n", [1, 2, 3, 65, 257, 4099])
def test_small_and_odd_shapes(cuda, n):
    from cdcmdr_amd.evaluate import eval_gauc, eval_metrics
    n_user = 8
    for q, kind in enumerate(("five", "distinct", "zeros")):
        rng = np.random.default_rng(1000 * n + q)
        s, sb = _scores(kind, n, rng), _scores(kind, n, rng)
        y = (rng.random(n) < 0.45).astype(np.int16)
        dom = rng.choice([0, 2], size=n).astype(np.int32)                    # 3 domains: 1 is empty ...
        u = rng.integers(0, n_user, size=n).astype(np.int32)
        y[u == 5] = 0                                                           # a user with a single class in domain 0
        y[dom == 2] = 1                                                         # ... and 2 holds one class
        w = (0.25 + rng.random(n_user)) if q != 1 else None
        strided = q != 2
        label, st = torch.from_numpy(y).to(cuda), torch.from_numpy(s).to(cuda)
        ut, dt = _columns(cuda, n, [u, dom], True)

        want = loss_ci_exact(y, s, sb, dom, 3)
        assert want[1]["rows"] == 0 and want[2]["loss"] is None
        got = _loss_device(cuda, y, s, sb, dom, 3, strided=strided)
        _check_loss(got, want, f"loss/{kind}/{n}/paired", err=_loss_err(s, sb))
        one = _loss_device(cuda, y, s, None, dom, 3, strided=strided)
        _check_loss(one, want, f"loss/{kind}/{n}", err=_loss_err(s))
        assert _bits(one, got, LOSS_KEYS[:2])                                   # pred_b changes nothing of a's
        loss = eval_metrics(st, label, dt, 3)[1].cpu().numpy()                  # eval_metrics' figure, bit for bit
        assert np.array_equal(loss.view(np.int64), got[0]["loss"].view(np.int64)), (kind, n, loss, got[0]["loss"])

        want = gauc_ci_exact(y, s, u, dom, 3, w, sb)
        assert want[1]["counted"] == want[2]["counted"] == 0 and want[2]["gauc"] is None
        got = _gauc_device(cuda, y, s, u, n_user, sb, dom, 3, w, strided=strided)
        _check_gauc(got, want, f"gauc/{kind}/{n}/paired")
        one = _gauc_device(cuda, y, s, u, n_user, None, dom, 3, w, strided=strided)
        _check_gauc(one, want, f"gauc/{kind}/{n}")
        assert _bits(one, got, GAUC_KEYS[:2])
        wt = None if w is None else torch.from_numpy(w).to(cuda)
        g, c, l = eval_gauc(st, label, ut, n_user, dt, 3, wt)                   # eval_gauc's figure, bit for bit
        assert np.array_equal(g.cpu().numpy().view(np.int64), got[0]["gauc"].view(np.int64)), (kind, n, g, got[0]["gauc"])
        assert c.cpu().numpy().tolist() == got[1].tolist() and l.cpu().numpy().tolist() == got[2].tolist()
    # no domain column: the one domain is every row
    _check_loss(_loss_device(cuda, y, s, sb), loss_ci_exact(y, s, sb), f"loss/{n}/no domain", err=_loss_err(s, sb))
    _check_gauc(_gauc_device(cuda, y, s, u, n_user, sb), gauc_ci_exact(y, s, u, None, 1, None, sb), f"gauc/{n}/no domain")


def test_zero_one_and_two_counted_users(cuda):
    s = np.array([0.3, 0.7, 0.5, 0.5, 0.1], dtype=np.float32)
    u = [0, 0, 1, 1, 2]
    for y, K in (([1, 1, 0, 0, 0], 0), ([0, 1, 1, 1, 0], 1), ([0, 1, 1, 0, 0], 2)):
        want = gauc_ci_exact(y, s, u, None, 1, None, -s + np.float32(1.0))
        assert want[1]["counted"] == K
        got = _gauc_device(cuda, y, s, u, 3, -s + np.float32(1.0))
        _check_gauc(got, want, f"K={K}")
        assert np.isnan(got[0]["gauc"]).all() == (K == 0) and np.isnan(got[0]["var"]).all() == (K < 2)
        assert np.isnan(got[0]["delta"]).all() == (K == 0) and np.isnan(got[0]["var_delta"]).all() == (K < 2)
    # K = 2, A = (1, 1/2), w = (2, 2): G = 3/4, var = 2 * (1/4 + 1/4) / 16 = 1/16, every step exact in binary
    got = _gauc_device(cuda, [0, 1, 1, 0, 0], s, u, 3)
    assert got[0]["gauc"].tolist() == [0.75, 0.75] and got[0]["var"].tolist() == [0.0625, 0.0625]
    # the log-loss of two rows: l = (log 2, -log 0.75), var = (l0 - l1)^2 / 4 from the centred pass
    got = _loss_device(cuda, [1, 0], np.array([0.5, 0.25], dtype=np.float32))
    _check_loss(got, loss_ci_exact([1, 0], np.array([0.5, 0.25], dtype=np.float32)), "two rows")
    assert abs(got[0]["var"][0] - (math.log(2.0) + math.log(0.75)) ** 2 / 4) <= 64 * U * got[0]["var"][0]


@functools.lru_cache(maxsize=None)
def _big():
    """70 001 rows, 7 domains of very unequal size (4 empty, 6 of 3 rows, 3 single-class), about 5 000 Zipf-distributed users: user 0
    holds about 12 000 rows — more than a slice (a 64th of a segment), a scan block and a workgroup's stretch — and most users
    one or two.  The second vector: the first with 300 rows nudged."""
    n, n_domain, n_user = 70_001, 7, 5000
    rng = np.random.default_rng(70_001)
    s = rng.random(n).astype(np.float32)
    s[rng.random(n) < 0.2] = np.float32(0.5)
    s[:4] = [-0.0, 0.0, 1e-42, 1.0 - 2 ** -24]
    y = (rng.random(n) < 0.3 + 0.3 * s).astype(np.int16)
    dom = rng.choice(n_domain, size=n, p=[0.55, 0.3, 0.1, 0.04, 0.0, 0.00996, 0.00004]).astype(np.int32)
    dom[dom == 6] = 5
    dom[[10, 20_000, 70_000]] = 6
    y[[10, 20_000, 70_000]] = [0, 1, 0]
    y[dom == 3] = 0
    u = ((rng.zipf(1.2, size=n) - 1) % n_user).astype(np.int32)
    u[:4] = 17                                                   # the signed zeros in one group
    y[:4] = [1, 0, 0, 1]
    dom[:4] = 1
    sb = s.copy()
    hit = rng.permutation(n)[:300]
    sb[hit] = np.clip(sb[hit] + (rng.random(300).astype(np.float32) - np.float32(0.5)) * np.float32(0.02), 0, 1).astype(np.float32)
    w = 0.1 + rng.random(n_user) * 5.0
    for a in (s, sb, y, dom, u, w):
        a.setflags(write=False)
    exact = {"loss": loss_ci_exact(y, s, sb, dom, n_domain), None: gauc_ci_exact(y, s, u, dom, n_domain, None, sb),
             "w": gauc_ci_exact(y, s, u, dom, n_domain, w, sb)}
    return n_domain, n_user, y, s, sb, dom, u, w, exact


def test_loss_segments_across_block_boundaries_and_the_paired_variance(cuda):
    from cdcmdr_amd.evaluate import eval_metrics
    n_domain, n_user, y, s, sb, dom, u, w, exact = _big()
    want = exact["loss"]
    assert want[4]["rows"] == 0 and want[6]["rows"] == 3 and want[3]["loss"] is None and want[3]["rows"] > 2000 and want[0]["rows"] > 35_000
    # the paired variance is far below either loss's own: var + var_b - 2 cov would have to cancel three of its digits
    for d in (0, 1, 2, n_domain):
        assert 0 < want[d]["var_delta"] < want[d]["var"] / 1000, (d, want[d]["var_delta"], want[d]["var"])
    got = _loss_device(cuda, y, s, sb, dom, n_domain, strided=True)
    _check_loss(got, want, "70k")
    loss = eval_metrics(torch.from_numpy(s).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(dom).to(cuda), n_domain)[1].cpu().numpy()
    assert np.array_equal(loss.view(np.int64), got[0]["loss"].view(np.int64))
    assert _bits(got, _loss_device(cuda, y, s, sb, dom, n_domain))              # the same call, contiguous columns: the same bits
    assert _bits(got, _loss_device(cuda, y, s, None, dom, n_domain), LOSS_KEYS[:2])
    # the rows in another order: other additions, the same bounds, and still eval_metrics' bits on those rows
    perm = np.random.default_rng(1).permutation(len(y))
    other = _loss_device(cuda, y[perm], s[perm], sb[perm], dom[perm], n_domain)
    _check_loss(other, want, "70k permuted")
    loss = eval_metrics(torch.from_numpy(s[perm]).to(cuda), torch.from_numpy(y[perm]).to(cuda), torch.from_numpy(dom[perm]).to(cuda),
                        n_domain)[1].cpu().numpy()
    assert np.array_equal(loss.view(np.int64), other[0]["loss"].view(np.int64))
    # the second vector equal to the first: zero, not merely small
    same = _loss_device(cuda, y, s, s.copy(), dom, n_domain)
    for d in range(n_domain + 1):
        if want[d]["var"] is not None:
            assert same[0]["var_delta"][d] == 0.0 and same[0]["delta"][d] == 0.0
    assert np.array_equal(same[0]["var_b"].view(np.int64), same[0]["var"].view(np.int64))
    assert np.isnan(got[0]["loss"]).sum() == 2 and np.isnan(got[0]["var"]).sum() == 2


@pytest.mark.parametrize("weighted", [False, True])
def test_gauc_groups_across_slice_and_block_boundaries(cuda, weighted):
    from cdcmdr_amd.evaluate import eval_gauc
    n_domain, n_user, y, s, sb, dom, u, w, exact = _big()
    want = exact["w" if weighted else None]
    ww = w if weighted else None
    assert int((u == 0).sum()) > 2 * len(y) // 64 and int((u == 0).sum()) > 4096    # one user beyond a slice of "all rows" and a block
    assert want[4]["counted"] == want[4]["left_out"] == 0 and want[3]["counted"] == 0 and want[3]["left_out"] > 100
    assert want[n_domain]["counted"] > 1500 and want[6]["var"] is None
    assert 0 < want[n_domain]["var_delta"] < want[n_domain]["var"] / 100
    got = _gauc_device(cuda, y, s, u, n_user, sb, dom, n_domain, ww, strided=True)
    _check_gauc(got, want, f"70k/{weighted}")
    ut, dt = _columns(cuda, len(y), [u, dom], False)
    g, c, l = eval_gauc(torch.from_numpy(s).to(cuda), torch.from_numpy(y).to(cuda), ut, n_user, dt, n_domain,
                        None if ww is None else torch.from_numpy(ww).to(cuda))
    assert np.array_equal(g.cpu().numpy().view(np.int64), got[0]["gauc"].view(np.int64))
    assert c.cpu().numpy().tolist() == got[1].tolist() and l.cpu().numpy().tolist() == got[2].tolist()
    assert _bits(got, _gauc_device(cuda, y, s, u, n_user, None, dom, n_domain, ww), GAUC_KEYS[:2])
    # the rows in another order: the same bits, NaN included
    perm = np.random.default_rng(1).permutation(len(y))
    assert _bits(got, _gauc_device(cuda, y[perm], s[perm], u[perm], n_user, sb[perm], dom[perm], n_domain, ww))
    if weighted:
        return
    # a strictly increasing transform of the scores, and the scores themselves: zero, not merely small
    mono = s * np.float32(0.5)                                  # exact, so ties stay ties and nothing else becomes one
    assert len(np.unique(mono + np.float32(0.0))) == len(np.unique(s + np.float32(0.0)))
    for other in (s.copy(), mono):
        same = _gauc_device(cuda, y, s, u, n_user, other, dom, n_domain, None)
        for d in range(n_domain + 1):
            if want[d]["var"] is not None:
                assert same[0]["var_delta"][d] == 0.0 and same[0]["delta"][d] == 0.0
        assert _bits(got, same, GAUC_KEYS[:2]) and np.array_equal(same[0]["var_b"].view(np.int64), same[0]["var"].view(np.int64))


def test_bad_rows_set_the_error_word(cuda):
    s = np.array([0.2, 0.3, 0.7, 0.6, 0.1], dtype=np.float32)
    y, u = [0, 1, 1, 0, 1], [0, 0, 1, 1, 2]
    assert _loss_device(cuda, y, s, s)[3] == 0 and _gauc_device(cuda, y, s, u, 3, s)[3] == 0
    bad = s.copy()
    bad[3] = np.nan
    assert _loss_device(cuda, y, s, bad)[3] == 4 and _gauc_device(cuda, y, s, u, 3, bad)[3] == 4        # a NaN in pred_b alone
    assert _loss_device(cuda, y, bad, s)[3] == 4 and _loss_device(cuda, y, bad)[3] == 4 and _gauc_device(cuda, y, bad, u, 3)[3] == 4
    out = s.copy()
    out[1] = 1.5
    assert _loss_device(cuda, y, out)[3] == 2 and _loss_device(cuda, y, s, out)[3] == 2                 # outside [0, 1]
    out[2] = -0.25
    assert _loss_device(cuda, y, out)[3] == 3
    assert _loss_device(cuda, [0, 1, 2, 0, 1], s)[3] == 3 and _gauc_device(cuda, [0, 1, 2, 0, 1], s, u, 3)[3] == 3     # label 2
    assert _loss_device(cuda, y, s, s, dom=[0, 1, 0, 1, 2], n_domain=2)[3] == 5                         # domain == n_domain
    assert _loss_device(cuda, y, s, None, dom=[0, -1, 0, 1, 1], n_domain=2)[3] == 2
    assert _gauc_device(cuda, y, s, u, 3, None, dom=[0, 1, 2, 0, 1], n_domain=2)[3] == 3
    assert _gauc_device(cuda, y, s, [0, 0, 1, 3, 2], 3)[3] == 4                                         # user == n_user
    assert _gauc_device(cuda, y, s, [0, 0, -1, 1, 2], 3, s)[3] == 3
    # a clamped user still indexes user_weight inside its bounds: it counts as user n_user - 1, whose weight is used
    wt = [1.0, 2.0, 3.0]
    got = _gauc_device(cuda, y, s, [0, 0, 1, 2 ** 31 - 1, 2], 3, s, w=wt, strided=True)
    assert got[3] == 4
    _check_gauc(got, gauc_ci_exact(y, s, [0, 0, 1, 2, 2], None, 1, wt, s), "clamped", err=4)


def _tiny(cuda):
    from cdcmdr_amd.model.mmoe import MMoE
    FD = [50, 50, 40, 3]                                        # column 2: 40 users, column 3: 3 domains
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


def test_evaluator_loss_ci_and_gauc_ci(cuda):
    from cdcmdr_amd.evaluate import Evaluator, _z, eval_gauc_ci, eval_loss_ci
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    kw = dict(mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w, user_idx=2, n_user=40)
    base = Evaluator(model, **kw)
    res0 = base.test(loader)
    assert sorted(res0) == ["domain_auc", "domain_gauc", "domain_loss", "mean_auc", "mean_gauc", "mean_loss", "total_auc", "total_gauc",
                            "total_loss"]                      # the flags off: today's keys
    ev = Evaluator(model, loss_ci=True, gauc_ci=True, **kw)
    res = ev.test(loader)
    assert sorted(res) == sorted(list(res0) + ["total_loss_se", "domain_loss_se", "mean_loss_se", "total_gauc_se", "domain_gauc_se"])
    for k in res0:
        assert res[k] == res0[k]                                # the other figures are untouched
    pred, label, dom, user = ev._score(loader)
    assert np.array_equal(label.cpu().numpy(), y) and np.array_equal(user.cpu().numpy(), X[:, 2])
    lv = eval_loss_ci(pred, label, dom, 3).var.cpu().tolist()   # the direct calls on the same predictions
    gv = eval_gauc_ci(pred, label, user, 40, dom, 3).var.cpu().tolist()
    assert res["total_loss_se"] == math.sqrt(lv[3]) > 0 and res["total_gauc_se"] == math.sqrt(gv[3]) > 0
    assert res["domain_loss_se"] == {d: math.sqrt(lv[d]) for d in range(3)} and res["domain_gauc_se"] == {d: math.sqrt(gv[d]) for d in range(3)}
    assert res["mean_loss_se"] == math.sqrt(sum(w[d] ** 2 * lv[d] for d in range(3)))
    want = loss_ci_exact(label.cpu().numpy(), pred.cpu().numpy(), None, dom.cpu().numpy(), 3)
    assert abs(lv[3] - want[3]["var"]) <= _loss_bounds(want[3])["var"]
    # per-domain evaluation off: the totals only
    res = Evaluator(model, loss_ci=True, gauc_ci=True, is_evaluate_multi_domain=False, **kw).test(loader)
    assert sorted(res) == ["total_auc", "total_gauc", "total_gauc_se", "total_loss", "total_loss_se"]

    # raw against Platt-recalibrated on one checkpoint: the AUC keys as before, and a log-loss delta that is not zero
    recal = base.fit_recalibration(loader, method="platt")
    other = Evaluator(model, recalibration=recal, **kw)
    auc_only = base.compare(other, loader)
    nine = ["domain_delta", "domain_delta_se", "domain_z", "mean_delta", "mean_delta_se", "mean_z", "total_delta", "total_delta_se", "total_z"]
    assert sorted(auc_only) == nine                             # the flags off: today's keys
    both = ev.compare(other, loader)
    assert sorted(both) == sorted(nine + [k.replace("delta", "loss_delta").replace("_z", "_loss_z") for k in nine] +
                                  ["total_gauc_delta", "total_gauc_delta_se", "total_gauc_z", "domain_gauc_delta", "domain_gauc_delta_se",
                                   "domain_gauc_z"])
    for k in nine:                                              # NaN (a z of 0 / 0) equals itself here
        assert repr(both[k]) == repr(auc_only[k]), (k, both[k], auc_only[k])
    assert both["total_loss_delta"] != 0.0 and both["total_loss_delta_se"] > 0 and math.isfinite(both["total_loss_z"])
    pb = other.predict(loader)[0]
    lci = eval_loss_ci(pred, label, dom, 3, pred_b=pb)
    gci = eval_gauc_ci(pred, label, user, 40, dom, 3, pred_b=pb)
    ld, lvd, gd, gvd = (t.cpu().tolist() for t in (lci.delta, lci.var_delta, gci.delta, gci.var_delta))
    assert both["total_loss_delta"] == ld[3] and both["total_loss_delta_se"] == math.sqrt(lvd[3])
    assert both["total_loss_z"] == ld[3] / math.sqrt(lvd[3])
    assert both["domain_loss_delta"] == {d: ld[d] for d in range(3)} and both["domain_loss_delta_se"] == {d: math.sqrt(lvd[d]) for d in range(3)}
    assert both["mean_loss_delta"] == sum(w[d] * ld[d] for d in range(3))
    assert both["mean_loss_delta_se"] == math.sqrt(sum(w[d] ** 2 * lvd[d] for d in range(3)))
    assert both["total_gauc_delta"] == gd[3] and both["total_gauc_delta_se"] == math.sqrt(gvd[3])
    assert both["domain_gauc_delta"] == {d: gd[d] for d in range(3)}
    for d in range(3):
        z, want_z = both["domain_gauc_z"][d], _z(gd[d], math.sqrt(gvd[d]))
        assert z == want_z or (z != z and want_z != want_z)
    want = loss_ci_exact(label.cpu().numpy(), pred.cpu().numpy(), pb.cpu().numpy(), dom.cpu().numpy(), 3)
    assert abs(lvd[3] - want[3]["var_delta"]) <= _loss_bounds(want[3])["var_delta"]
    # the other evaluator without the user column: compare() says so
    with pytest.raises(ValueError, match="different user columns"):
        ev.compare(Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w), loader)
