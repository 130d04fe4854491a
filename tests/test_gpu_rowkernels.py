"""The small element-wise and row kernels of csrc/rowops.hip, csrc/attention.hip and csrc/misc.hip straight through the C-ABI against
float64 (or, where the operation is exact in fp32, bit for bit against the same fp32 operation on the CPU), with the conventions
of tests/test_gpu_head.py: padded buffers (NaN in input padding, a sentinel that must survive in output padding), accumulate
targets pre-filled with random values and plain stores with NaN, bounds derived from the float64 terms (helpers.sum_bound) and
capped by the suite's present figures, cross-row sums run twice for bit equality.  Every kernel gets one shape whose element
count passes its grid cap, so that the grid-stride loop makes a second trip.  Last: csrc/embedding.hip's cdc_embed_lazy_update,
which no other test calls, bit for bit against the fused launch that training uses."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import (OUT_FIG, SUM_FIG, U24, PadBuf, assert_bits_equal, assert_bounded, capped, host_ulps, nan_like, sum_bound, ulp32)

pytestmark = pytest.mark.gpu

EW = [(1, 1), (7, 63), (257, 65), (100, 130)]
BIG4096 = (4100, 257)                           # > 4096 blocks x 256 threads
BIG8192 = (8200, 257)                           # > 8192 x 256
SUM_B, SUM_E = [1, 255, 256, 257, 1000], [1, 64, 65, 416]
BADARG, TOOBIG = -1, -2


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


def rnd(rng, *shape, scale=1.0):
    return f32(scale * rng.standard_normal(shape))


def exact32(v64):
    """A single fp32 operation on fp32 operands is the float64 result rounded once."""
    return np.asarray(v64, dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# DCN cross layer: out = x0 (xl . w) + b + xl
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", SUM_E)
@pytest.mark.parametrize("B", SUM_B)
def test_cross_fwd_bwd(cuda, lib, B, E):
    rng = np.random.default_rng(1000 * B + E)
    x0, xl, w, b = rnd(rng, B, E), rnd(rng, B, E), rnd(rng, E, scale=E ** -0.5), rnd(rng, E, scale=0.3)
    dout, dx0_old = rnd(rng, B, E, scale=0.1 / B), rnd(rng, B, E)              # the upstream gradient of a mean loss: O(1 / B)
    X0, XL, W, Bv = PadBuf(cuda, x0), PadBuf(cuda, xl), PadBuf(cuda, w), PadBuf(cuda, b)
    s = d64(xl) @ d64(w)
    a_s = np.abs(d64(xl)) @ np.abs(d64(w))
    want = d64(x0) * s[:, None] + d64(b)[None, :] + d64(xl)
    bound = capped(sum_bound(np.abs(d64(x0)) * a_s[:, None] + np.abs(d64(b))[None, :] + np.abs(d64(xl)), E, 3), want, OUT_FIG)
    saves = []
    for save in (True, False):
        out, xw = PadBuf(cuda, nan_like(B, E), out=True), PadBuf(cuda, nan_like(1, B), out=True)
        call(lib, "cdc_cross_fwd", X0.ptr, X0.ld, XL.ptr, XL.ld, W.ptr, Bv.ptr, out.ptr, out.ld, xw.ptr if save else None, B, E)
        assert_bounded(out.read("cross out"), want, bound, f"cross_fwd out (xw_save {save})")
        saves.append(xw.read("xw_save"))
    assert_bounded(saves[0], s.reshape(1, B), capped(sum_bound(a_s, E, 0), s, OUT_FIG).reshape(1, B), "cross_fwd xw_save")
    assert np.isnan(saves[1]).all()                                              # NULL: nothing stored anywhere near
    # backward from the kernel's own fp32 xw_save
    s32 = d64(saves[0][0])
    ds, a_ds = np.sum(d64(dout) * d64(x0), 1), np.sum(np.abs(d64(dout) * d64(x0)), 1)
    w_dx0 = d64(dx0_old) + d64(dout) * s32[:, None]
    w_dxl = d64(dout) + ds[:, None] * d64(w)[None, :]
    b_dxl = np.abs(d64(w))[None, :] * sum_bound(a_ds, E, 0)[:, None] + 2 * U24 * (np.abs(d64(dout)) + np.abs(ds[:, None] * d64(w)[None, :]))
    w_dw, w_db = ds @ d64(xl), d64(dout).sum(0)
    runs = []
    for _ in range(2):
        DO, S = PadBuf(cuda, dout), PadBuf(cuda, saves[0])
        dx0, dxl = PadBuf(cuda, dx0_old, out=True), PadBuf(cuda, nan_like(B, E), out=True)
        dw, db = PadBuf(cuda, nan_like(1, E), out=True), PadBuf(cuda, nan_like(1, E), out=True)
        ws = torch.full((256 * 2 * E,), float("nan"), device=cuda)
        call(lib, "cdc_cross_bwd", DO.ptr, DO.ld, X0.ptr, X0.ld, XL.ptr, XL.ld, W.ptr, S.ptr, dx0.ptr, dx0.ld, dxl.ptr, dxl.ld, dw.ptr, db.ptr,
             ws.data_ptr(), B, E)
        runs.append([dx0.read("d_x0"), dxl.read("d_xl"), dw.read("dw"), db.read("db")])
    for a, b2, nm in zip(runs[0], runs[1], ("d_x0", "d_xl", "dw", "db")):
        assert_bits_equal(a, b2, f"cross_bwd {nm}: two runs")
    g = runs[0]
    assert_bounded(g[0], w_dx0, capped(2 * U24 * (np.abs(d64(dx0_old)) + np.abs(d64(dout) * s32[:, None])), w_dx0, OUT_FIG), "cross_bwd d_x0 +=")
    assert_bounded(g[1], w_dxl, capped(b_dxl, w_dxl, OUT_FIG), "cross_bwd d_xl")
    assert_bounded(g[2], w_dw.reshape(1, E), capped(sum_bound(a_ds @ np.abs(d64(xl)), B + E, 1), w_dw, SUM_FIG).reshape(1, E), "cross_bwd dw")
    assert_bounded(g[3], w_db.reshape(1, E), capped(sum_bound(np.abs(d64(dout)).sum(0), B, 0), w_db, SUM_FIG).reshape(1, E), "cross_bwd db")


def test_cross_bwd_rejects_wide_rows(cuda, lib):
    t = torch.zeros(4 * 2049 + 8, device=cuda)
    p = t.data_ptr()
    assert lib.cdc_cross_bwd(p, 2049, p, 2049, p, 2049, p, p, p, 2049, p, 2049, p, p, p, 1, 2049, _stream()) == TOOBIG
    assert b"cross_bwd: E too large" in lib.cdc_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# DCN-v2 combine: out[:, kP+e] = x0[:, e] (u[:, kP+e] + b1[e]) + b2[e] + r[:, kP+e]
# ------------------------------------------------------------------------------------------------------------------------
# (b1, b2, r present; d_r present, accumulate_r; db1 / db2 present; accumulate_b1, accumulate_b2)
COMBINE_CFG = [
    dict(b1=1, b2=1, r=1, d_r=1, acc_r=1, db1=1, db2=1, acc1=1, acc2=0),
    dict(b1=0, b2=1, r=0, d_r=0, acc_r=0, db1=0, db2=1, acc1=0, acc2=1),
    dict(b1=1, b2=0, r=1, d_r=1, acc_r=0, db1=1, db2=0, acc1=0, acc2=0),
    dict(b1=0, b2=0, r=0, d_r=0, acc_r=0, db1=0, db2=0, acc1=0, acc2=0),       # neither: the final launch is skipped
    dict(b1=1, b2=1, r=0, d_r=1, acc_r=1, db1=1, db2=1, acc1=0, acc2=1),
    dict(b1=1, b2=1, r=1, d_r=0, acc_r=0, db1=1, db2=1, acc1=1, acc2=1),
]
_COMBINE_SHAPES = [(B, P, n) for B in SUM_B for P in SUM_E for n in (1, 4)]
_COMBINE = [(B, P, n, (i + j) % 6) for i, (B, P, n) in enumerate(_COMBINE_SHAPES) for j in (0, 3)] + \
           [(r, c, 1, i % 6) for i, (r, c) in enumerate(EW + [BIG4096])] + [(7, 63, 4, 0), (100, 130, 4, 4)]


@pytest.mark.parametrize("rows,P,n_rep,cfg", _COMBINE)
def test_cross_combine_fwd_bwd(cuda, lib, rows, P, n_rep, cfg):
    c = COMBINE_CFG[cfg]
    rng = np.random.default_rng(rows * 7919 + P * 31 + n_rep + cfg)
    cols = P * n_rep
    x0, u, dout = rnd(rng, rows, P), rnd(rng, rows, cols), rnd(rng, rows, cols, scale=0.1 / rows)     # (a mean loss's gradient)
    b1, b2, r = rnd(rng, P, scale=0.5), rnd(rng, P, scale=0.5), rnd(rng, rows, cols)
    dx0_old, dr_old, db1_old, db2_old = rnd(rng, rows, P), rnd(rng, rows, cols), rnd(rng, P), rnd(rng, P)
    X0, U = PadBuf(cuda, x0), PadBuf(cuda, u)
    B1, B2, R = (PadBuf(cuda, b1) if c["b1"] else None), (PadBuf(cuda, b2) if c["b2"] else None), (PadBuf(cuda, r) if c["r"] else None)
    ptr = lambda b: None if b is None else b.ptr
    x0t = np.tile(d64(x0), (1, n_rep))
    ub = d64(u) + (np.tile(d64(b1), n_rep)[None, :] if c["b1"] else 0.0)
    a_ub = np.abs(d64(u)) + (np.tile(np.abs(d64(b1)), n_rep)[None, :] if c["b1"] else 0.0)
    want = x0t * ub + (np.tile(d64(b2), n_rep)[None, :] if c["b2"] else 0.0) + (d64(r) if c["r"] else 0.0)
    mag = np.abs(x0t) * a_ub + (np.tile(np.abs(d64(b2)), n_rep)[None, :] if c["b2"] else 0.0) + (np.abs(d64(r)) if c["r"] else 0.0)
    out = PadBuf(cuda, nan_like(rows, cols), out=True)
    call(lib, "cdc_cross_combine_fwd", X0.ptr, X0.ld, U.ptr, U.ld, ptr(B1), ptr(B2), ptr(R), R.ld if R else 0, out.ptr, out.ld, rows, P, n_rep)
    assert_bounded(out.read("combine out"), want, capped(4 * U24 * mag, want, OUT_FIG), "cross_combine_fwd out")
    # backward
    do = d64(dout)
    w_du = do * x0t
    per_k = (do * ub).reshape(rows, n_rep, P)
    w_dx0 = d64(dx0_old) + per_k.sum(1)
    b_dx0 = sum_bound(np.abs(d64(dx0_old)) + (np.abs(do) * a_ub).reshape(rows, n_rep, P).sum(1), n_rep, 3)
    w_dr = (d64(dr_old) if c["acc_r"] else 0.0) + do
    w_db1 = (d64(db1_old) if c["acc1"] else 0.0) + w_du.reshape(rows, n_rep, P).sum((0, 1))
    w_db2 = (d64(db2_old) if c["acc2"] else 0.0) + do.reshape(rows, n_rep, P).sum((0, 1))
    m_db1 = (np.abs(d64(db1_old)) if c["acc1"] else 0.0) + np.abs(w_du).reshape(rows, n_rep, P).sum((0, 1))
    m_db2 = (np.abs(d64(db2_old)) if c["acc2"] else 0.0) + np.abs(do).reshape(rows, n_rep, P).sum((0, 1))
    runs = []
    for _ in range(2):
        DO = PadBuf(cuda, dout)
        du, dx0 = PadBuf(cuda, nan_like(rows, cols), out=True), PadBuf(cuda, dx0_old, out=True)
        dr = PadBuf(cuda, dr_old if c["acc_r"] else nan_like(rows, cols), out=True) if c["d_r"] else None
        db1 = PadBuf(cuda, db1_old if c["acc1"] else nan_like(1, P), out=True) if c["db1"] else None
        db2 = PadBuf(cuda, db2_old if c["acc2"] else nan_like(1, P), out=True) if c["db2"] else None
        ws = torch.full((256 * 2 * P,), float("nan"), device=cuda)
        call(lib, "cdc_cross_combine_bwd", DO.ptr, DO.ld, X0.ptr, X0.ld, U.ptr, U.ld, ptr(B1), du.ptr, du.ld, dx0.ptr, dx0.ld, ptr(dr),
             dr.ld if dr else 0, c["acc_r"], ptr(db1), c["acc1"], ptr(db2), c["acc2"], ws.data_ptr(), rows, P, n_rep)
        runs.append({k: b.read(k) for k, b in (("d_u", du), ("d_x0", dx0), ("d_r", dr), ("db1", db1), ("db2", db2)) if b is not None})
    for k in runs[0]:
        assert_bits_equal(runs[0][k], runs[1][k], f"cross_combine_bwd {k}: two runs")
    g = runs[0]
    assert_bits_equal(g["d_u"], exact32(w_du), "cross_combine_bwd d_u (one product)")
    assert_bounded(g["d_x0"], w_dx0, capped(b_dx0, w_dx0, OUT_FIG), "cross_combine_bwd d_x0 +=")
    if c["d_r"]:
        assert_bits_equal(g["d_r"], exact32(w_dr), "cross_combine_bwd d_r (copy or one addition)")
    if c["db1"]:
        assert_bounded(g["db1"], w_db1.reshape(1, P), capped(sum_bound(m_db1, rows * n_rep, 2), w_db1, SUM_FIG).reshape(1, P), "cross_combine_bwd db1")
    if c["db2"]:
        assert_bounded(g["db2"], w_db2.reshape(1, P), capped(sum_bound(m_db2, rows * n_rep, 1), w_db2, SUM_FIG).reshape(1, P), "cross_combine_bwd db2")


# ------------------------------------------------------------------------------------------------------------------------
# tanh
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", EW + [BIG4096])
def test_tanh_fwd_bwd(cuda, lib, rows, cols):
    rng = np.random.default_rng(rows + cols)
    x = rnd(rng, rows, cols, scale=2.0)
    x.flat[::5] = f32(rng.uniform(-12, 12, size=x.flat[::5].shape))             # saturation: y = +-1 exactly, 1 - y^2 = 0
    x.flat[:2] = (12.0, -12.0)[:x.size]
    dy, old = rnd(rng, rows, cols), rnd(rng, rows, cols)
    X, Y = PadBuf(cuda, x), PadBuf(cuda, nan_like(rows, cols), out=True)
    call(lib, "cdc_tanh_fwd", X.ptr, X.ld, Y.ptr, Y.ld, rows, cols)
    y = Y.read("tanh y")
    want = np.tanh(d64(x))
    # tanhf on the host over these inputs against float64: 1.4 ulp of the result at worst (measured; asserted here); allowed 4x = 5.6 ulp
    TANH_ULPS_HOST = 1.4
    assert host_ulps(np.tanh(x), want) <= TANH_ULPS_HOST
    assert_bounded(y, want, capped(4 * TANH_ULPS_HOST * ulp32(want), want, OUT_FIG), "tanh_fwd")
    assert (np.abs(y[np.abs(x) >= 10]) == 1).all()
    yv = d64(y)
    v = d64(dy) * (1.0 - yv * yv)
    b = np.abs(d64(dy)) * U24 * (yv * yv + np.abs(1.0 - yv * yv)) + U24 * np.abs(v)     # y^2, 1 - y^2, the product
    for acc in (0, 1):
        DY, YY, DX = PadBuf(cuda, dy), PadBuf(cuda, y), PadBuf(cuda, old if acc else nan_like(rows, cols), out=True)
        call(lib, "cdc_tanh_bwd", DY.ptr, DY.ld, YY.ptr, YY.ld, DX.ptr, DX.ld, rows, cols, acc)
        w = (d64(old) if acc else 0.0) + v
        assert_bounded(DX.read("tanh dx"), w, capped(b + (U24 * np.abs(w) if acc else 0.0), w, OUT_FIG), f"tanh_bwd accumulate={acc}")


# ------------------------------------------------------------------------------------------------------------------------
# sigmoid gate: pi = beta sigmoid(alpha p), 0 where |pi| <= eps; out = a pi
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta,alpha,eps", [(2.0, 1.0, 0.25), (2.0, 1.0, -1.0)], ids=["adasparse", "pepnet"])
@pytest.mark.parametrize("rows,cols", EW + [BIG8192])
def test_sigmoid_gate_fwd_bwd(cuda, lib, rows, cols, beta, alpha, eps):
    rng = np.random.default_rng(rows * 131 + cols)
    p = rnd(rng, rows, cols, scale=2.0) - np.float32(1.5)
    for _ in range(4):                                                           # drawn so that no gate lies within 1e-4 of the threshold
        s = 1.0 / (1.0 + np.exp(-alpha * d64(p)))                                # (float64): a draw that close is moved down by 0.01,
        close = np.abs(np.abs(beta * s) - eps) <= 2e-4                           # which moves pi by 2e-3; every element is compared
        p = np.where(close, p - np.float32(0.01), p).astype(np.float32)
    s = 1.0 / (1.0 + np.exp(-alpha * d64(p)))
    assert (np.abs(np.abs(beta * s) - eps) > 1e-4).all()
    pruned = np.abs(beta * s) <= eps
    if eps > 0 and rows * cols > 100:
        assert pruned.any() and (~pruned).any()
    a, dout, old_a, old_p = rnd(rng, rows, cols), rnd(rng, rows, cols), rnd(rng, rows, cols), rnd(rng, rows, cols)
    a[a == 0] = 1.0
    pi = np.where(pruned, 0.0, beta * s)
    # beta / (1 + expf(-alpha p)) on the host against float64: 3.3 ulp at worst (measured; asserted); allowed 4x = 13.2 ulp
    GATE_ULPS_HOST = 3.3
    with np.errstate(over="ignore"):
        host = np.float32(beta) / (np.float32(1) + np.exp(np.float32(-alpha) * p))
    assert host_ulps(host, beta * s) <= GATE_ULPS_HOST
    d_pi = 4 * GATE_ULPS_HOST * ulp32(pi)
    A, Pb = PadBuf(cuda, a), PadBuf(cuda, p)
    out = PadBuf(cuda, nan_like(rows, cols), out=True)
    call(lib, "cdc_sigmoid_gate_fwd", A.ptr, A.ld, Pb.ptr, Pb.ld, out.ptr, out.ld, rows, cols, beta, alpha, eps)
    got = out.read("gate out")
    assert np.array_equal(got == 0, pruned), "sigmoid_gate_fwd: pruned mask"
    w_out = d64(a) * pi
    assert_bounded(got, w_out, capped(np.abs(d64(a)) * d_pi + U24 * np.abs(w_out), w_out, OUT_FIG), "sigmoid_gate_fwd out")
    g = d64(dout)
    v_a = g * pi
    b_a = np.abs(g) * d_pi + 2 * U24 * np.abs(v_a)
    ds = 4 * GATE_ULPS_HOST * ulp32(s)
    v_p = np.where(pruned, 0.0, g * d64(a) * beta * alpha * s * (1.0 - s))
    b_p = np.where(pruned, 0.0, np.abs(g * d64(a) * beta * alpha) * ds * (np.abs(1.0 - 2.0 * s) + ds) + 7 * U24 * np.abs(v_p))
    DO = PadBuf(cuda, dout)
    for which in ("a", "p", "both"):
        for acc in (0, 1):
            da = PadBuf(cuda, old_a if acc else nan_like(rows, cols), out=True) if which != "p" else None
            dp = PadBuf(cuda, old_p if acc else nan_like(rows, cols), out=True) if which != "a" else None
            call(lib, "cdc_sigmoid_gate_bwd", A.ptr, A.ld, Pb.ptr, Pb.ld, DO.ptr, DO.ld, da.ptr if da else None, da.ld if da else 0, acc,
                 dp.ptr if dp else None, dp.ld if dp else 0, acc, rows, cols, beta, alpha, eps)
            if da:
                w = (d64(old_a) if acc else 0.0) + v_a
                assert_bounded(da.read("da"), w, capped(b_a + (U24 * np.abs(w) if acc else 0.0), w, OUT_FIG), f"sigmoid_gate_bwd da ({which}, acc {acc})")
            if dp:
                w = (d64(old_p) if acc else 0.0) + v_p
                gp = dp.read("dp")
                assert_bounded(gp, w, capped(b_p + (U24 * np.abs(w) if acc else 0.0), w, OUT_FIG), f"sigmoid_gate_bwd dp ({which}, acc {acc})")
                if not acc:
                    assert (gp[pruned] == 0).all(), "sigmoid_gate_bwd: pruned gates pass no gradient"


# ------------------------------------------------------------------------------------------------------------------------
# group select (exact: a choice of elements)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_group,H", [(B, n, H) for B in (1, 7, 257, 100) for n in (1, 3, 50) for H in (1, 65)] + [(8200, 3, 257)])
def test_group_select_fwd_bwd(cuda, lib, B, n_group, H):
    rng = np.random.default_rng(B * 100 + n_group + H)
    feas, dout, old = rnd(rng, B, n_group * H), rnd(rng, B, H), rnd(rng, B, n_group * H)
    grp = rng.integers(0, n_group, size=B).astype(np.int64)
    if B >= 3:
        grp[1], grp[B - 1] = -1, n_group                                        # outside: zeros forward, nothing backward
    G = torch.from_numpy(grp).to(cuda)
    ok = (grp >= 0) & (grp < n_group)
    idx = np.where(ok, grp, 0)[:, None] * H + np.arange(H)[None, :]
    want = np.where(ok[:, None], np.take_along_axis(feas, idx, 1), np.float32(0))
    F, out = PadBuf(cuda, feas), PadBuf(cuda, nan_like(B, H), out=True)
    call(lib, "cdc_group_select_fwd", F.ptr, F.ld, G.data_ptr(), out.ptr, out.ld, B, n_group, H)
    assert_bits_equal(out.read("group_select out"), want, "group_select_fwd")
    scat = np.zeros((B, n_group * H), dtype=np.float32)
    np.put_along_axis(scat, idx, np.where(ok[:, None], dout, np.float32(0)), 1)
    chosen = np.zeros((B, n_group * H), dtype=bool)
    np.put_along_axis(chosen, idx, np.broadcast_to(ok[:, None], (B, H)), 1)
    DO = PadBuf(cuda, dout)
    for acc in (0, 1):
        df = PadBuf(cuda, old if acc else nan_like(B, n_group * H), out=True)
        call(lib, "cdc_group_select_bwd", DO.ptr, DO.ld, G.data_ptr(), df.ptr, df.ld, B, n_group, H, acc)
        got = df.read("group_select dfeas")
        if acc:
            assert_bits_equal(got, np.where(chosen, old + scat, old), "group_select_bwd accumulate: one addition in the chosen block")
        else:
            assert_bits_equal(got, scat, "group_select_bwd: zeros in the unchosen blocks")


# ------------------------------------------------------------------------------------------------------------------------
# relu(a + b) and the exact element-wise kernels
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", EW + [BIG8192])
def test_add_relu_fwd_bwd(cuda, lib, rows, cols):
    rng = np.random.default_rng(rows * 3 + cols)
    a, b, dout, old_a, old_b = (rnd(rng, rows, cols) for _ in range(5))
    a.flat[::7] = 0.0
    b.flat[::11] = 0.0
    b.flat[::5] = -a.flat[::5]                                                   # a + b == 0 exactly (incl. 0 + 0 at multiples of 35)
    A, Bb, out = PadBuf(cuda, a), PadBuf(cuda, b), PadBuf(cuda, nan_like(rows, cols), out=True)
    call(lib, "cdc_add_relu_fwd", A.ptr, A.ld, Bb.ptr, Bb.ld, out.ptr, out.ld, rows, cols)
    y = out.read("add_relu out")
    assert_bits_equal(y, np.maximum(exact32(d64(a) + d64(b)), np.float32(0)) + np.float32(0), "add_relu_fwd (one addition)")
    d = np.where(y > 0, dout, np.float32(0))                                     # the header's mask: out > 0
    Y, DO = PadBuf(cuda, y), PadBuf(cuda, dout)
    for acc_a in (0, 1):
        for acc_b in (0, 1):
            da = PadBuf(cuda, old_a if acc_a else nan_like(rows, cols), out=True)
            db = PadBuf(cuda, old_b if acc_b else nan_like(rows, cols), out=True)
            call(lib, "cdc_add_relu_bwd", Y.ptr, Y.ld, DO.ptr, DO.ld, da.ptr, da.ld, acc_a, db.ptr, db.ld, acc_b, rows, cols)
            assert_bits_equal(da.read("da"), old_a + d if acc_a else d, f"add_relu_bwd da (acc {acc_a}, {acc_b})")
            assert_bits_equal(db.read("db"), old_b + d if acc_b else d, f"add_relu_bwd db (acc {acc_a}, {acc_b})")


@pytest.mark.parametrize("rows,cols", EW + [BIG4096])
def test_add_out_and_copy_or_add(cuda, lib, rows, cols):
    rng = np.random.default_rng(rows * 5 + cols)
    a, b, old = rnd(rng, rows, cols), rnd(rng, rows, cols), rnd(rng, rows, cols)
    A, Bb, out = PadBuf(cuda, a), PadBuf(cuda, b), PadBuf(cuda, nan_like(rows, cols), out=True)
    call(lib, "cdc_add_out", A.ptr, A.ld, Bb.ptr, Bb.ld, out.ptr, out.ld, rows, cols)
    assert_bits_equal(out.read("add_out"), a + b, "add_out")
    for acc in (0, 1):
        dst = PadBuf(cuda, old if acc else nan_like(rows, cols), out=True)
        call(lib, "cdc_copy_or_add", dst.ptr, dst.ld, A.ptr, A.ld, rows, cols, acc)
        assert_bits_equal(dst.read("copy_or_add"), old + a if acc else a, f"copy_or_add accumulate={acc}")


@pytest.mark.parametrize("rows,cols,n_slices", [(r, c, n) for r, c in EW for n in (1, 3, 50)] + [BIG4096 + (3,)])
def test_sum_slices(cuda, lib, rows, cols, n_slices):
    rng = np.random.default_rng(rows + cols + n_slices)
    x, old = rnd(rng, rows, cols * n_slices), rnd(rng, rows, cols)
    acc32 = np.zeros((rows, cols), dtype=np.float32)
    for g in range(n_slices):
        acc32 = acc32 + x[:, g * cols:(g + 1) * cols]                            # fp32, slice order
    X = PadBuf(cuda, x)
    for acc in (0, 1):
        out = PadBuf(cuda, old if acc else nan_like(rows, cols), out=True)
        call(lib, "cdc_sum_slices", X.ptr, X.ld, out.ptr, out.ld, rows, cols, n_slices, acc)
        assert_bits_equal(out.read("sum_slices"), old + acc32 if acc else acc32, f"sum_slices accumulate={acc}")


# ------------------------------------------------------------------------------------------------------------------------
# STAR parameter fusion
# ------------------------------------------------------------------------------------------------------------------------
def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("op", [0, 1], ids=["mul", "add"])
@pytest.mark.parametrize("n,size", [(1, 1), (3, 16705), (30, 1000), (3, 300000), (1, 600000), (3, 600000)])
def test_star_fuse_fwd_bwd(cuda, lib, op, n, size):
    from cdcmdr_amd import _lib as L
    rng = np.random.default_rng(n * 10 + size + op)
    s, a, dout, ds_old = rnd(rng, size), rnd(rng, n, size), rnd(rng, n, size), rnd(rng, size)
    S = _dev(cuda, s)
    Aa = [_dev(cuda, a[g]) for g in range(n)]
    outs = [torch.full((size + 3,), float("nan"), device=cuda) for _ in range(n)]
    args = L.StarFuseArgs()
    args.n, args.op, args.size, args.s = n, op, size, S.data_ptr()
    for g in range(n):
        args.a[g], args.out[g] = Aa[g].data_ptr(), outs[g].data_ptr()
    call(lib, "cdc_star_fuse_fwd", C.byref(args))
    for g in range(n):
        o = outs[g].cpu().numpy()
        assert np.isnan(o[size:]).all(), "star_fuse_fwd wrote past the tensor"
        assert_bits_equal(o[:size], a[g] * s if op == 0 else a[g] + s, f"star_fuse_fwd domain {g} (one operation)")
    do = d64(dout)
    terms = do * d64(a) if op == 0 else do
    for acc, with_ds, skip in ((0, True, ()), (1, True, (0,)), (0, False, (n - 1,))):
        DO = [_dev(cuda, dout[g]) for g in range(n)]
        da = [None if g in skip else torch.full((size + 3,), float("nan"), device=cuda) for g in range(n)]
        ds = _dev(cuda, np.concatenate([ds_old if acc else nan_like(1, size)[0], nan_like(1, 3)[0]])) if with_ds else None
        b = L.StarFuseArgs()
        b.n, b.op, b.size, b.s, b.accumulate_ds = n, op, size, S.data_ptr(), acc
        b.ds = ds.data_ptr() if with_ds else None
        for g in range(n):
            b.a[g], b.out[g] = Aa[g].data_ptr(), DO[g].data_ptr()
            b.da[g] = None if da[g] is None else da[g].data_ptr()
        call(lib, "cdc_star_fuse_bwd", C.byref(b))
        for g in range(n):
            if da[g] is not None:
                o = da[g].cpu().numpy()
                assert np.isnan(o[size:]).all()
                assert_bits_equal(o[:size], dout[g] * s if op == 0 else dout[g], f"star_fuse_bwd da[{g}]")
        if with_ds:
            o = ds.cpu().numpy()
            assert np.isnan(o[size:]).all()
            w = (d64(ds_old) if acc else 0.0) + terms.sum(0)
            m = (np.abs(d64(ds_old)) if acc else 0.0) + np.abs(terms).sum(0)
            assert_bounded(o[:size], w, capped(sum_bound(m, n, (1 if op == 0 else 0) + acc), w, SUM_FIG), f"star_fuse_bwd ds (accumulate {acc})")


def test_star_fuse_rejects_bad_counts(cuda, lib):
    from cdcmdr_amd import _lib as L
    t = torch.zeros(8, device=cuda)
    for n in (0, L.MAX_GROUPS + 1):
        a = L.StarFuseArgs()
        a.n, a.op, a.size, a.s = n, 0, 8, t.data_ptr()
        for g in range(L.MAX_GROUPS):
            a.a[g], a.out[g] = t.data_ptr(), t.data_ptr()
        for fn, nm in ((lib.cdc_star_fuse_fwd, b"star_fuse_fwd"), (lib.cdc_star_fuse_bwd, b"star_fuse_bwd")):
            assert fn(C.byref(a), _stream()) == BADARG
            assert nm + b": bad argument" in lib.cdc_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# BCE on the mean of a row's tower probabilities
# ------------------------------------------------------------------------------------------------------------------------
def _bce_row(x, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        la, lb = np.maximum(np.log1p(-x), -100.0), np.maximum(np.log(x), -100.0)
    return (t - 1.0) * la - t * lb, np.abs((t - 1.0) * la) + np.abs(t * lb)


def _bce_grad(x, t, inv, n_col):
    return inv * (x - t) / np.maximum((1.0 - x) * x, 1e-12) / n_col


@pytest.mark.parametrize("with_dp", [True, False])
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("n_col", [1, 3, 8])
@pytest.mark.parametrize("B", [1, 1000, 4097])
def test_bce_mean_fwd_bwd(cuda, lib, B, n_col, kind, with_dp):
    rng = np.random.default_rng(B + n_col)
    p = f32(rng.uniform(0.02, 0.98, size=(B, n_col)))
    y = rng.integers(0, 2, size=B)
    if B >= 8:
        p[0], p[1], p[2], p[3] = 0.0, 1.0, 0.0, 1.0                              # means exactly 0 and 1: both clamps, with either label
        y[:4] = (0, 0, 1, 1)
    if kind == "f32":
        y = np.where(rng.random(B) < 0.25, rng.random(B), y)
    y = y.astype(np.int16 if kind == "i16" else np.float32)
    t, inv = d64(y), 1.0 / B
    x = d64(p).sum(1) / n_col
    dx = sum_bound(x, n_col, 1)                                                  # the fp32 mean: n_col additions and the division
    lo, hi = np.clip(x - dx, 0.0, 1.0), np.clip(x + dx, 0.0, 1.0)
    rows, mag = _bce_row(x, t)
    # the row formula in fp32 on the host against float64 (from the fp32 mean): 2.8 ulp of the terms' magnitudes at worst
    # (measured; asserted below); allowed 4x = 11.2 ulp.  The loss is convex in the mean: its change over [x - dx, x + dx]
    # is largest at an end.
    LOSS_ULPS_HOST = 2.8
    x32, y32 = (p.sum(1, dtype=np.float32) / np.float32(n_col)).astype(np.float32), y.astype(np.float32)
    with np.errstate(divide="ignore"):
        host = (y32 - np.float32(1)) * np.maximum(np.log1p(-x32), np.float32(-100)) - y32 * np.maximum(np.log(x32), np.float32(-100))
    r32, m32 = _bce_row(d64(x32), t)
    assert float(np.max(np.abs(d64(host) - r32) / ulp32(m32))) <= LOSS_ULPS_HOST
    prop = np.maximum(np.abs(_bce_row(lo, t)[0] - rows), np.abs(_bce_row(hi, t)[0] - rows))
    loss = rows.sum() * inv
    b_loss = inv * np.sum(prop + 4 * LOSS_ULPS_HOST * ulp32(mag)) + 2 * U24 * abs(loss)
    g = _bce_grad(x, t, inv, n_col)
    b_g = np.maximum(np.abs(_bce_grad(lo, t, inv, n_col) - g), np.abs(_bce_grad(hi, t, inv, n_col) - g)) + 8 * U24 * np.abs(g)
    P, Y = PadBuf(cuda, p), torch.from_numpy(y).to(cuda)
    dp = PadBuf(cuda, nan_like(B, n_col), out=True) if with_dp else None
    out = torch.full((1,), float("nan"), device=cuda)
    call(lib, "cdc_bce_mean_fwd_bwd", P.ptr, P.ld, Y.data_ptr() if kind == "i16" else None, Y.data_ptr() if kind == "f32" else None,
         out.data_ptr(), dp.ptr if dp else None, dp.ld if dp else 0, B, n_col, inv)
    assert_bounded(out.cpu().numpy(), np.array([loss]), capped(np.array([b_loss]), loss, OUT_FIG), "bce_mean loss")
    if dp:
        want = np.repeat(g[:, None], n_col, 1)
        assert_bounded(dp.read("bce_mean dp"), want, capped(np.repeat(b_g[:, None], n_col, 1), want, OUT_FIG), "bce_mean dp")


# ------------------------------------------------------------------------------------------------------------------------
# out[i] = a[i] b[i % nb] and its gradients
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,reps", [(nb, r) for nb in (1, 64, 65, 416, 600) for r in (1, 30, 255, 256, 257, 1000)])
def test_mul_bcast_fwd_bwd(cuda, lib, nb, reps):
    rng = np.random.default_rng(nb * 1000 + reps)
    na = nb * reps                                                               # (600, 1000): 600 000 elements, past the grid cap
    a, b, dout = rnd(rng, reps, nb), rnd(rng, nb), rnd(rng, reps, nb, scale=0.1 / reps)   # (a mean over the reps)
    A, Bb, DO = _dev(cuda, a), _dev(cuda, b), _dev(cuda, dout)
    out = torch.full((na + 3,), float("nan"), device=cuda)
    call(lib, "cdc_mul_bcast", A.data_ptr(), Bb.data_ptr(), out.data_ptr(), na, nb)
    o = out.cpu().numpy()
    assert np.isnan(o[na:]).all()
    assert_bits_equal(o[:na].reshape(reps, nb), a * b[None, :], "mul_bcast (one product)")
    w_db = np.sum(d64(dout) * d64(a), 0)
    b_db = capped(sum_bound(np.sum(np.abs(d64(dout) * d64(a)), 0), reps, 0), w_db, SUM_FIG)
    got_db = []
    for with_da, with_db in ((True, True), (False, True), (True, False)):
        da = torch.full((na + 3,), float("nan"), device=cuda) if with_da else None
        db = torch.full((nb + 3,), float("nan"), device=cuda) if with_db else None
        call(lib, "cdc_mul_bcast_bwd", DO.data_ptr(), A.data_ptr(), Bb.data_ptr(), da.data_ptr() if with_da else None,
             db.data_ptr() if with_db else None, na, nb)
        if with_da:
            o = da.cpu().numpy()
            assert np.isnan(o[na:]).all()
            assert_bits_equal(o[:na].reshape(reps, nb), dout * b[None, :], "mul_bcast_bwd da (one product)")
        if with_db:
            o = db.cpu().numpy()
            assert np.isnan(o[nb:]).all()
            assert_bounded(o[:nb], w_db, b_db, "mul_bcast_bwd db")
            got_db.append(o[:nb])
    assert_bits_equal(got_db[0], got_db[1], "mul_bcast_bwd db: two runs")


def test_mul_bcast_rejects_ragged(cuda, lib):
    t = torch.zeros(16, device=cuda)
    p = t.data_ptr()
    assert lib.cdc_mul_bcast(p, p, p, 10, 3, _stream()) == BADARG and b"mul_bcast: bad argument" in lib.cdc_last_error()
    assert lib.cdc_mul_bcast_bwd(p, p, p, p, p, 10, 3, _stream()) == BADARG and b"mul_bcast_bwd: bad argument" in lib.cdc_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# the lazy table's row update from stored gradient sums (csrc/embedding.hip): cdc_embed_lazy_update after cdc_embed_segment_sum
# against the launch that forms a row's sum and uses it on the spot
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 6], ids=["float4", "scalar"])
def test_lazy_update_from_rowgrad_equals_segsum_lazy_update(cuda, lib, D):
    """sort_dedupe -> segment_sum -> lazy_update against segsum_lazy_update (short_only = 0) from a copy of the same table: the same
    arithmetic in the same order (segments under 64 entries are summed serially in ascending order by both), so w, m, v and last
    are equal bit for bit, and rows outside the batch keep their values.  Vocabularies 4, 40 and 100000 give segments of about
    24, of a few and of one entry; one id per field is -1 (a padding entry: skipped by both)."""
    from cdcmdr_amd import _lib as L
    from cdcmdr_amd.optim import step_scalar_table
    B, F, t = 96, 3, 3
    vocab = (4, 40, 100000)
    offsets = np.concatenate([[0], np.cumsum(vocab)[:-1]])
    R = int(np.sum(vocab))
    rng = np.random.default_rng(7 + D)
    idx = np.stack([offsets[f] + rng.integers(0, vocab[f], size=B) for f in range(F)], axis=1).astype(np.int32)
    for f in range(F):
        idx[11 * f + 5, f] = -1
    w0, m0 = rnd(rng, R, D, scale=0.1), rnd(rng, R, D, scale=0.01)
    v0 = f32(1e-4 * rng.random((R, D)))
    d_out = _dev(cuda, rnd(rng, B, F * D, scale=0.05))
    scalars = step_scalar_table(1e-3, 0.9, 0.99, n=16).to(cuda).contiguous()
    hp = L.AdamHP()
    hp.lerp_w, hp.beta2, hp.one_minus_beta2, hp.eps = (float(np.float32(x)) for x in (1 - 0.9, 0.99, 1 - 0.99, 1e-8))
    hp.weight_decay, hp.l2_twice = float(np.float32(1e-8)), 2.0 * float(np.float32(1e-5))
    hp.step_scalars, hp.n_scalars = scalars.data_ptr(), scalars.shape[0]
    step_dev = torch.full((1,), t, dtype=torch.int32, device=cuda)
    d_idx = _dev(cuda, idx)
    uniq = torch.full((F, B), -7, dtype=torch.int32, device=cuda)
    seg = torch.full((F, B + 1), -7, dtype=torch.int32, device=cuda)
    perm = torch.full((F, B), -7, dtype=torch.int32, device=cuda)
    cnt = torch.zeros(F, dtype=torch.int32, device=cuda)
    call(lib, "cdc_embed_sort_dedupe", d_idx.data_ptr(), uniq.data_ptr(), seg.data_ptr(), perm.data_ptr(), cnt.data_ptr(), None, B, F)
    lens = [np.diff(seg[f, :int(cnt[f]) + 1].cpu().numpy()) for f in range(F)]
    assert 8 <= lens[0][:4].min() and lens[0][:4].max() < 64 and lens[2].max() <= 2          # the segment classes the docstring names

    def table():
        return [_dev(cuda, a) for a in (w0, m0, v0)] + [torch.full((R,), t - 1, dtype=torch.int32, device=cuda)]

    wa, ma, va, la = table()
    rowgrad = torch.full((F, B, D), float("nan"), device=cuda)
    call(lib, "cdc_embed_segment_sum", d_out.data_ptr(), seg.data_ptr(), perm.data_ptr(), cnt.data_ptr(), None, rowgrad.data_ptr(), B, F, D)
    call(lib, "cdc_embed_lazy_update", rowgrad.data_ptr(), uniq.data_ptr(), cnt.data_ptr(), wa.data_ptr(), ma.data_ptr(), va.data_ptr(),
         la.data_ptr(), hp, step_dev.data_ptr(), None, 0, B, F, D)
    wb, mb, vb, lb = table()
    call(lib, "cdc_embed_segsum_lazy_update", d_out.data_ptr(), seg.data_ptr(), perm.data_ptr(), cnt.data_ptr(), uniq.data_ptr(),
         wb.data_ptr(), mb.data_ptr(), vb.data_ptr(), lb.data_ptr(), hp, step_dev.data_ptr(), B, F, D, 0)
    for a, b, nm in ((wa, wb, "w"), (ma, mb, "m"), (va, vb, "v")):
        assert_bits_equal(a.cpu().numpy(), b.cpu().numpy(), f"lazy_update {nm}: rowgrad round trip against the sum used on the spot")
    assert np.array_equal(la.cpu().numpy(), lb.cpu().numpy())
    touched = np.zeros(R, dtype=bool)
    touched[idx[idx >= 0]] = True
    assert touched.sum() > F and not touched.all()
    assert np.array_equal(la.cpu().numpy(), np.where(touched, t, t - 1).astype(np.int32))
    for a, a0, nm in ((wa, w0, "w"), (ma, m0, "m"), (va, v0, "v")):
        got = a.cpu().numpy()
        assert_bits_equal(got[~touched], a0[~touched], f"lazy_update {nm}: rows outside the batch")
        assert (got[touched] != a0[touched]).any(), f"lazy_update {nm}: the batch's rows moved"
