"""The weighted stand-alone loss launches (csrc/rowops.hip cdc_bce_weighted_fwd_bwd, cdc_bce_mean_weighted_fwd_bwd) and the launch
that forms a step's effective row weights (cdc_stage_weights), straight through the C-ABI.

The two loss launches against float64 in the manner of tests/test_gpu_rowkernels.py::test_bce_mean_fwd_bwd, with its bound
construction: the row terms of its loss and gradient bounds are scaled by the row's weight, and one more fp32 rounding is allowed
for the weight itself (the loss adds (double)l * (double)w, the gradient is the finished unweighted value times w).  Then the bit
equalities the contract states: all-ones weights are the unweighted entry point, a uniform weight 4 is the unweighted entry point
called with 4 * inv_count (a power of two scales every operation exactly), a row of weight 0 has an all-zero gradient row.

cdc_stage_weights is exact in fp32 — w = (row * dom) * pos, two roundings in a fixed order — and is compared bit for bit with the same
expression in numpy."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import OUT_FIG, OUT_SENTINEL, U24, PadBuf, assert_bits_equal, assert_bounded, capped, nan_like, sum_bound, ulp32

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 4099]                        # 4099: more than one round of 4 rows x 1024 threads
# the fp32 row formula on the host against float64, in ulps of the two terms' magnitudes: 3.18 at worst over the cases of this file
# (asserted in reference(); test_bce_mean_fwd_bwd measures 2.8 over its rows, tests/tower_ref.py 3.43 over its own and allows 3.5);
# allowed 4 x, the device's logf / log1pf need not match the host's last bits
LOSS_ULPS_HOST = 3.5


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    from cdcmdr_amd import _lib as L
    L.check(getattr(lib, name)(*args, _stream()), name)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def d64(a):
    return np.asarray(a, dtype=np.float64)


def _bce_row(x, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        la, lb = np.maximum(np.log1p(-x), -100.0), np.maximum(np.log(x), -100.0)
    return (t - 1.0) * la - t * lb, np.abs((t - 1.0) * la) + np.abs(t * lb)


def _bce_grad(x, t, inv, n_col):
    return inv * (x - t) / np.maximum((1.0 - x) * x, 1e-12) / n_col


def make_weights(seed, B):
    """seeded uniform [0, 3), every eighth exactly 0, one 2^-20 and one 1024"""
    w = f32(np.random.default_rng(seed).uniform(0.0, 3.0, size=B))
    w[7::8] = 0.0
    w[B - 1] = 1024.0
    if B >= 2:
        w[B - 2] = 2.0 ** -20
    return w


def make_inputs(B, n_col, kind):
    rng = np.random.default_rng(1000 * B + n_col)
    p = f32(rng.uniform(0.02, 0.98, size=(B, n_col)))
    y = rng.integers(0, 2, size=B)
    edge_p, edge_y = (0.0, 1.0, 0.0, 1.0), (0, 0, 1, 1)          # probabilities exactly 0 and 1 with either label: both clamps, the floor
    for r in range(min(B, 4)):
        p[r], y[r] = edge_p[r], edge_y[r]
    if kind == "f32":
        soft = rng.random(B) < 0.25
        soft[:4] = False
        y = np.where(soft, rng.random(B), y)
    return p, y.astype(np.int16 if kind == "i16" else np.float32), rng


def groups(rng, B, n_col):
    """NULL, random, and with -1 / n_col among valid values (both go to column 0)"""
    g_rand = rng.integers(0, n_col, size=B).astype(np.int64)
    g_out = g_rand.copy()
    g_out[0::3] = -1
    g_out[1::3] = n_col
    return [("null", None), ("random", g_rand), ("outside", g_out)]


def reference(p, y, w, group, inv, mean):
    """float64 loss and gradient with their bounds: test_bce_mean_fwd_bwd's construction, the row terms times w, one rounding more"""
    B, n_col = p.shape
    t, wd = d64(y), d64(w)
    if mean:
        x = d64(p).sum(1) / n_col
        dx = sum_bound(x, n_col, 1)                               # the fp32 mean: n_col additions and the division
        col, div = None, n_col
    else:
        col = np.zeros(B, dtype=np.int64) if group is None else np.where((group < 0) | (group >= n_col), 0, group)
        x = d64(p)[np.arange(B), col]                             # the gathered probability is exact
        dx = np.zeros(B)
        div = 1
    lo, hi = np.clip(x - dx, 0.0, 1.0), np.clip(x + dx, 0.0, 1.0)
    rows, mag = _bce_row(x, t)
    x32 = (p.sum(1, dtype=np.float32) / np.float32(n_col)).astype(np.float32) if mean else p[np.arange(B), col]
    y32 = y.astype(np.float32)
    with np.errstate(divide="ignore"):
        host = (y32 - np.float32(1)) * np.maximum(np.log1p(-x32), np.float32(-100)) - y32 * np.maximum(np.log(x32), np.float32(-100))
    r32, m32 = _bce_row(d64(x32), t)
    assert float(np.max(np.abs(d64(host) - r32) / ulp32(m32))) <= LOSS_ULPS_HOST
    prop = np.maximum(np.abs(_bce_row(lo, t)[0] - rows), np.abs(_bce_row(hi, t)[0] - rows))
    loss = float(np.sum(wd * rows) * inv)
    b_loss = inv * np.sum(wd * (prop + 4 * LOSS_ULPS_HOST * ulp32(mag)) + U24 * wd * mag) + 2 * U24 * abs(loss)
    g0 = _bce_grad(x, t, inv, div)
    g = g0 * wd
    b_g = wd * np.maximum(np.abs(_bce_grad(lo, t, inv, div) - g0), np.abs(_bce_grad(hi, t, inv, div) - g0)) + (8 + 1) * U24 * np.abs(g)
    if mean:
        want, bound = np.repeat(g[:, None], n_col, 1), np.repeat(b_g[:, None], n_col, 1)
    else:
        want, bound = np.zeros((B, n_col)), np.zeros((B, n_col))
        want[np.arange(B), col], bound[np.arange(B), col] = g, b_g
    return loss, b_loss, want, bound


def run(lib, cuda, p, y, group, w, inv, mean, with_dp):
    """one launch (w None: the unweighted entry point) -> (loss fp32 [1], dp or None); padded leading dimensions, sentinels checked"""
    B, n_col = p.shape
    P, Y = PadBuf(cuda, p), torch.from_numpy(y).to(cuda)
    G = None if group is None else torch.from_numpy(group).to(cuda)
    W = None if w is None else torch.from_numpy(f32(w)).to(cuda)
    dp = PadBuf(cuda, nan_like(B, n_col), out=True) if with_dp else None
    out = torch.full((1,), float("nan"), device=cuda)
    yi, yf = (Y.data_ptr(), None) if y.dtype == np.int16 else (None, Y.data_ptr())
    tail = (out.data_ptr(), dp.ptr if dp else None, dp.ld if dp else 0, B, n_col, inv)
    if mean:
        head = (P.ptr, P.ld, yi, yf)
        name = "cdc_bce_mean_fwd_bwd" if w is None else "cdc_bce_mean_weighted_fwd_bwd"
    else:
        head = (P.ptr, P.ld, None if G is None else G.data_ptr(), yi, yf)
        name = "cdc_bce_fwd_bwd" if w is None else "cdc_bce_weighted_fwd_bwd"
    call(lib, name, *head, *(() if w is None else (W.data_ptr(),)), *tail)
    return out.cpu().numpy(), (dp.read(name + " dp") if dp else None)


def check_case(lib, cuda, B, n_col, kind, mean):
    p, y, rng = make_inputs(B, n_col, kind)
    w = make_weights(B + 17 * n_col, B)
    inv = float(np.float32(1.0 / B))
    for gname, group in ([("mean", None)] if mean else groups(rng, B, n_col)):
        what = f"{'mean' if mean else 'gather'} B={B} n_col={n_col} {kind} group={gname}"
        loss, b_loss, want, bound = reference(p, y, w, group, inv, mean)
        for with_dp in (True, False):
            got_loss, got_dp = run(lib, cuda, p, y, group, w, inv, mean, with_dp)
            assert_bounded(got_loss, np.array([loss]), capped(np.array([b_loss]), loss, OUT_FIG), what + " loss")
            if with_dp:
                assert_bounded(got_dp, want, capped(bound, want, OUT_FIG), what + " dp")
                zero = w == 0
                assert np.all(got_dp[zero] == 0.0), what + ": a row of weight 0 has a gradient"
        # all-ones weights are the unweighted entry point, loss and gradient
        plain_loss, plain_dp = run(lib, cuda, p, y, group, None, inv, mean, True)
        ones_loss, ones_dp = run(lib, cuda, p, y, group, np.ones(B), inv, mean, True)
        assert_bits_equal(ones_loss, plain_loss, what + " loss, all-ones weights")
        assert_bits_equal(ones_dp, plain_dp, what + " dp, all-ones weights")
        # a uniform weight 4 is the unweighted entry point with 4 * inv_count
        four_loss, four_dp = run(lib, cuda, p, y, group, np.full(B, 4.0), inv, mean, True)
        scaled_loss, scaled_dp = run(lib, cuda, p, y, group, None, 4.0 * inv, mean, True)
        assert_bits_equal(four_loss, scaled_loss, what + " loss, uniform weight 4")
        assert_bits_equal(four_dp, scaled_dp, what + " dp, uniform weight 4")


@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("n_col", [1, 3])
@pytest.mark.parametrize("B", SIZES)
def test_bce_weighted_fwd_bwd(cuda, lib, B, n_col, kind):
    check_case(lib, cuda, B, n_col, kind, mean=False)


@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("n_col", [1, 3])
@pytest.mark.parametrize("B", SIZES)
def test_bce_mean_weighted_fwd_bwd(cuda, lib, B, n_col, kind):
    check_case(lib, cuda, B, n_col, kind, mean=True)


# ------------------------------------------------------------------------------------------------------------------------
# w[b] = (row[b] * domain_w[ids[b, col]]) * (y[b] > 0 ? pos_weight : 1)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", ["none", "row", "domain", "pos"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 4099])
def test_stage_weights(cuda, lib, B, absent):
    rng = np.random.default_rng(B)
    F, PADC, col, n_dom, TAIL = 5, 3, 2, 7, 8
    ids = np.full((B, F + PADC), -12345, dtype=np.int32)          # the domain column inside a padded ids matrix
    ids[:, :F] = rng.integers(0, 1000, size=(B, F))
    ids[:, col] = rng.integers(0, n_dom, size=B)
    outside = B // 2
    ids[outside, col] = n_dom if B % 2 else -1                    # one id outside the table: that row weighs 0
    row = make_weights(B + 5, B)
    dom_w = f32(rng.uniform(0.25, 4.0, size=n_dom))
    y = rng.integers(0, 2, size=B).astype(np.int16)
    pos = np.float32(2.5)
    have_row, have_dom, have_pos = absent != "row", absent != "domain", absent != "pos"
    r = row if have_row else np.ones(B, dtype=np.float32)
    if have_dom:
        idc = ids[:, col]
        inside = (idc >= 0) & (idc < n_dom)
        d = np.where(inside, dom_w[np.clip(idc, 0, n_dom - 1)], np.float32(0)).astype(np.float32)
    else:
        d = np.ones(B, dtype=np.float32)
    q = np.where(y > 0, pos, np.float32(1)).astype(np.float32) if have_pos else np.ones(B, dtype=np.float32)
    want = ((r * d).astype(np.float32) * q).astype(np.float32)
    if have_dom:
        assert want[outside] == 0.0
    Row, Ids, Dom, Y = (torch.from_numpy(a).to(cuda) for a in (row, ids, dom_w, y))
    out = torch.full((B + TAIL,), OUT_SENTINEL, dtype=torch.float32, device=cuda)
    call(lib, "cdc_stage_weights", Row.data_ptr() if have_row else None, Ids.data_ptr(), F + PADC, col,
         Dom.data_ptr() if have_dom else None, n_dom if have_dom else 0, Y.data_ptr() if have_pos else None,
         float(pos) if have_pos else 1.0, out.data_ptr(), B)
    got = out.cpu().numpy()
    assert_bits_equal(got[:B], want, f"stage_weights B={B} without {absent}")
    assert np.all(got[B:] == np.float32(OUT_SENTINEL)), "elements past B were written"
