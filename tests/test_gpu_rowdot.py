"""cdc_rowdot_fwd / cdc_rowdot_bwd (csrc/rowops.hip) straight through the C-ABI against float64 (tests/interaction_ref.py; the fused
BCE against tests/weighted_ref.py's head_backward without weights), with the conventions of tests/test_gpu_head.py.  Groups of
K = 1, 64 and 130 in one launch (a lane's first, full and third trip; the LDS accumulators of the backward are strided by
kmax + 1 = 131), outputs, addends, logits and d_out as columns of padded buffers, a NULL bias, ragged rows with an empty and a
one-row group, row counts that leave the backward's 256 parts empty, uneven or at a second four-row round, every optional
pointer NULL and set, the workspace and the loss partials poisoned with NaN, cross-row sums run twice for equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import interaction_ref as I
import weighted_ref as W
from helpers import PadBuf, assert_bits_equal, assert_bounded, nan_like

pytestmark = pytest.mark.gpu

KS = (1, 64, 130)
PARTS = 256                                     # CDC_ROWDOT_PARTS
RAGGED = (0, 0, 1, 40)                          # an empty group, a one-row group, the rest
BADARG = -1
f32 = lambda a: np.asarray(a, dtype=np.float32)


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _rows(offsets, g, M):
    return slice(0, M) if offsets is None else slice(offsets[g], offsets[g + 1])


def inputs(rng, M, Ks):
    return dict(x=[f32(rng.standard_normal((M, K))) for K in Ks], w=[f32(rng.standard_normal(K) / np.sqrt(K)) for K in Ks],
                b=[f32(0.3 * rng.standard_normal(1)) for _ in Ks])


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def run_forward(cuda, lib, M, Ks, D, adds, sigmoid, with_logit, offsets=None, null_bias=(1,)):
    """one launch; returns (out [M, n], logit [M, n] or None), columns of padded buffers pre-filled with NaN"""
    from cdcmdr_amd import _lib as L
    n = len(Ks)
    a = L.RowdotFwdArgs()
    keep = []
    k = lambda b: keep.append(b) or b
    a.n_groups, a.sigmoid, a.n_addend, a.M = n, sigmoid, len(adds), M
    if adds:
        AD = k(PadBuf(cuda, np.stack(adds, 1)))
        for i in range(len(adds)):
            a.addend[i], a.ld_addend[i] = AD.ptr + 4 * i, AD.ld
    if offsets is not None:
        a.row_offsets = k(_dev(cuda, np.asarray(offsets, dtype=np.int32))).data_ptr()
    out = PadBuf(cuda, nan_like(M, n), out=True)
    logit = PadBuf(cuda, nan_like(M, n), out=True)
    for g, K in enumerate(Ks):
        G = a.g[g]
        X, Wt = k(PadBuf(cuda, D["x"][g])), k(PadBuf(cuda, D["w"][g]))
        G.x, G.ldx, G.w, G.K = X.ptr, X.ld, Wt.ptr, K
        if g not in null_bias:
            G.bias = k(PadBuf(cuda, D["b"][g])).ptr
        G.out, G.ld_out = out.ptr + 4 * g, out.ld
        if with_logit:
            G.logit, G.ld_logit = logit.ptr + 4 * g, logit.ld
    L.check(lib.cdc_rowdot_fwd(C.byref(a), _stream()), "cdc_rowdot_fwd")
    lg = logit.read("rowdot logit")
    if not with_logit:
        assert np.isnan(lg).all()
    return out.read("rowdot out"), (lg if with_logit else None)


def check_forward(got, logit, M, Ks, D, adds, sigmoid, offsets, null_bias, what):
    for g, K in enumerate(Ks):
        r = _rows(offsets, g, M)
        want = I.rowdot_forward(D["x"][g][r], D["w"][g], None if g in null_bias else D["b"][g][0], [ad[r] for ad in adds], sigmoid)
        assert_bounded(got[r, g], want["out"][0], want["out"][1], f"{what} out, group {g} (K {K})")
        outside = np.ones(M, dtype=bool)
        outside[r] = False
        assert np.isnan(got[outside, g]).all(), f"{what}: group {g} wrote rows outside its range"
        if logit is not None:
            assert_bounded(logit[r, g], want["logit"][0], want["logit"][1], f"{what} logit, group {g} (K {K})")
            assert np.isnan(logit[outside, g]).all()


@pytest.mark.parametrize("sigmoid", [0, 1])
@pytest.mark.parametrize("with_logit", [0, 1])
@pytest.mark.parametrize("n_add", [0, 4])
@pytest.mark.parametrize("M", [1, 5, 257])
def test_rowdot_fwd_against_float64(cuda, lib, M, n_add, with_logit, sigmoid):
    rng = np.random.default_rng(M * 100 + n_add * 10 + with_logit * 2 + sigmoid)
    D = inputs(rng, M, KS)
    adds = [f32(0.5 * rng.standard_normal(M)) for _ in range(n_add)]
    out, logit = run_forward(cuda, lib, M, KS, D, adds, sigmoid, with_logit)
    check_forward(out, logit, M, KS, D, adds, sigmoid, None, (1,), f"rowdot_fwd M={M}")


@pytest.mark.parametrize("sigmoid", [0, 1])
def test_rowdot_fwd_ragged_and_full_group_list(cuda, lib, sigmoid):
    from cdcmdr_amd import _lib as L
    M = RAGGED[-1]
    rng = np.random.default_rng(40 + sigmoid)
    D = inputs(rng, M, KS)
    adds = [f32(0.5 * rng.standard_normal(M)) for _ in range(2)]
    out, logit = run_forward(cuda, lib, M, KS, D, adds, sigmoid, 1, RAGGED)
    check_forward(out, logit, M, KS, D, adds, sigmoid, RAGGED, (1,), "rowdot_fwd ragged")
    # CDC_MAX_GROUPS groups in one launch
    Ks = tuple(KS[g % 3] for g in range(L.MAX_GROUPS))
    D = inputs(rng, 5, Ks)
    null_bias = tuple(range(1, L.MAX_GROUPS, 3))
    out, logit = run_forward(cuda, lib, 5, Ks, D, [adds[0][:5]], sigmoid, 1, None, null_bias)
    check_forward(out, logit, 5, Ks, D, [adds[0][:5]], sigmoid, None, null_bias, "rowdot_fwd 32 groups")


# ------------------------------------------------------------------------------------------------------------------------
# plain backward
# ------------------------------------------------------------------------------------------------------------------------
# per group: dx NULL / stored / accumulated, dlogit, dw, dbias; rotated over the groups by the test's `rot`
CFG = (dict(dx=None, dlogit=1, dw=1, dbias=0), dict(dx="store", dlogit=0, dw=0, dbias=1), dict(dx="acc", dlogit=1, dw=1, dbias=1))


def run_backward(cuda, lib, M, Ks, D, dout, out32, cfgs, sigmoid, offsets=None, bce=None):
    """one launch with the workspace (and the loss partials) poisoned; returns name -> array of what exists.
    bce = dict(y, group or None, inv): the fused loss instead of d_out."""
    from cdcmdr_amd import _lib as L
    n = len(Ks)
    a = L.RowdotBwdArgs()
    keep = []
    k = lambda b: keep.append(b) or b
    a.n_groups, a.sigmoid, a.M = n, sigmoid, M
    if offsets is not None:
        a.row_offsets = k(_dev(cuda, np.asarray(offsets, dtype=np.int32))).data_ptr()
    a.workspace = k(torch.full((n * PARTS * (max(Ks) + 1),), float("nan"), device=cuda)).data_ptr()
    DO = k(PadBuf(cuda, dout)) if dout is not None else None
    O = k(PadBuf(cuda, out32)) if out32 is not None else None
    dlogit = PadBuf(cuda, nan_like(M, n), out=True)
    res = {}
    for g, K in enumerate(Ks):
        G, c = a.g[g], cfgs[g]
        X, Wt = k(PadBuf(cuda, D["x"][g])), k(PadBuf(cuda, D["w"][g]))
        G.x, G.ldx, G.w, G.K = X.ptr, X.ld, Wt.ptr, K
        if DO is not None:
            G.dout, G.ld_dout = DO.ptr + 4 * g, DO.ld
        if O is not None:
            G.out, G.ld_out = O.ptr + 4 * g, O.ld
        if c["dx"]:
            res[f"dx{g}"] = PadBuf(cuda, D["dx0"][g] if c["dx"] == "acc" else nan_like(M, K), out=True)
            G.dx, G.lddx, G.accumulate_dx = res[f"dx{g}"].ptr, res[f"dx{g}"].ld, int(c["dx"] == "acc")
        if c["dlogit"]:
            G.dlogit, G.ld_dlogit = dlogit.ptr + 4 * g, dlogit.ld
        if c["dw"]:
            res[f"dw{g}"] = PadBuf(cuda, nan_like(1, K), out=True)
            G.dw = res[f"dw{g}"].ptr
        if c["dbias"]:
            res[f"dbias{g}"] = PadBuf(cuda, nan_like(1, 1), out=True)
            G.dbias = res[f"dbias{g}"].ptr
    loss = torch.full((1,), float("nan"), device=cuda)
    if bce:
        y = k(_dev(cuda, bce["y"]))
        if bce["y"].dtype == np.int16:
            a.bce_y_i16 = y.data_ptr()
        else:
            a.bce_y_f32 = y.data_ptr()
        if bce["group"] is not None:
            a.bce_group = k(_dev(cuda, bce["group"])).data_ptr()
        a.bce_loss = loss.data_ptr()
        a.bce_partial = k(torch.full((n * PARTS,), float("nan"), dtype=torch.float64, device=cuda)).data_ptr()
        a.bce_inv_count = bce["inv"]
    L.check(lib.cdc_rowdot_bwd(C.byref(a), _stream()), "cdc_rowdot_bwd")
    got = {nm: b.read(nm) for nm, b in res.items()}
    got["dlogit"] = dlogit.read("dlogit")
    if bce:
        got["loss"] = loss.cpu().numpy()
    else:
        assert bool(torch.isnan(loss).all())
    return got


def check_backward(got, M, Ks, D, dout, out32, cfgs, sigmoid, offsets, what):
    for g, K in enumerate(Ks):
        c, r = cfgs[g], _rows(offsets, g, M)
        outside = np.ones(M, dtype=bool)
        outside[r] = False
        want = I.rowdot_backward(D["x"][g][r], D["w"][g], dout[r, g], out32[r, g] if sigmoid else None, sigmoid,
                                 D["dx0"][g][r] if c["dx"] == "acc" else None)
        if c["dx"]:
            assert_bounded(got[f"dx{g}"][r], want["dx"][0], want["dx"][1], f"{what} dx, group {g} (K {K}, {c['dx']})")
            untouched = D["dx0"][g] if c["dx"] == "acc" else nan_like(M, K)
            assert_bits_equal(got[f"dx{g}"][outside], untouched[outside], f"{what} dx, group {g}: rows outside its range")
        else:
            assert f"dx{g}" not in got
        if c["dlogit"]:
            assert_bounded(got["dlogit"][r, g:g + 1], want["dlogit"][0], want["dlogit"][1], f"{what} dlogit, group {g}")
            assert np.isnan(got["dlogit"][outside, g]).all()
        else:
            assert np.isnan(got["dlogit"][:, g]).all(), f"{what}: dlogit of group {g} written through a NULL pointer's neighbour"
        if c["dw"]:
            assert_bounded(got[f"dw{g}"], want["dw"][0], want["dw"][1], f"{what} dw, group {g} (K {K})")
        if c["dbias"]:
            assert_bounded(got[f"dbias{g}"], want["dbias"][0], want["dbias"][1], f"{what} dbias, group {g} (K {K})")


def _backward_case(cuda, lib, M, sigmoid, rot, offsets=None):
    rng = np.random.default_rng(M * 10 + sigmoid * 3 + rot)
    D = inputs(rng, M, KS)
    D["dx0"] = [f32(rng.standard_normal((M, K))) for K in KS]
    dout = f32(rng.standard_normal((M, len(KS))) / M)                           # the upstream gradient of a mean loss
    out32 = f32(rng.uniform(0.02, 0.98, size=(M, len(KS))))
    cfgs = [CFG[(g + rot) % 3] for g in range(len(KS))]
    runs = [run_backward(cuda, lib, M, KS, D, dout, out32 if sigmoid else None, cfgs, sigmoid, offsets) for _ in range(2)]
    assert set(runs[0]) == set(runs[1])
    for nm in runs[0]:
        assert_bits_equal(runs[0][nm], runs[1][nm], f"rowdot_bwd {nm}: two runs")
    check_backward(runs[0], M, KS, D, dout, out32, cfgs, sigmoid, offsets, f"rowdot_bwd M={M} sigmoid={sigmoid}")


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("sigmoid", [0, 1])
@pytest.mark.parametrize("M", [1, 16, 255, 256, 257, 4113])
def test_rowdot_bwd_against_float64(cuda, lib, M, sigmoid, rot):
    """257 rows: two per part, 127 parts empty and the last used one with a single row; 4113: 17 per part, a second four-row round
    that ends in a partial one."""
    _backward_case(cuda, lib, M, sigmoid, rot)


@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("sigmoid", [0, 1])
def test_rowdot_bwd_ragged(cuda, lib, sigmoid, rot):
    _backward_case(cuda, lib, RAGGED[-1], sigmoid, rot, RAGGED)


# ------------------------------------------------------------------------------------------------------------------------
# fused BCE, unweighted
# ------------------------------------------------------------------------------------------------------------------------
ALL = [dict(dx="store", dlogit=1, dw=1, dbias=1)] * 3


@pytest.mark.parametrize("gkind", ["none", "valid", "outside"])
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("M", [3, 257, 1030])
def test_rowdot_fused_bce_against_float64(cuda, lib, M, kind, gkind):
    n = len(KS)
    rng = np.random.default_rng(M + 7 * len(kind) + len(gkind))
    D = inputs(rng, M, KS)
    y = rng.integers(0, 2, size=M)
    if kind == "f32":
        y = np.where(rng.random(M) < 0.25, rng.random(M), y)
    D["y"] = y.astype(np.int16 if kind == "i16" else np.float32)
    grp = None if gkind == "none" else rng.integers(0, n, size=M).astype(np.int64)
    if gkind == "outside":
        grp[0::5] = -1                                                          # both act as column 0
        grp[2::7] = n
    D["group"] = grp
    out32 = f32(rng.uniform(0.02, 0.98, size=(M, n)))
    out32[0], out32[1], out32[M - 1] = 1.0, 0.0, (0.0, 1.0, 0.0)               # both clamps of the loss (-100) and the 1e-12 floor
    bce = dict(y=D["y"], group=grp, inv=1.0 / M)
    runs = [run_backward(cuda, lib, M, KS, D, None, out32, ALL, 1, None, bce) for _ in range(2)]
    for nm in runs[0]:
        assert_bits_equal(runs[0][nm], runs[1][nm], f"rowdot fused BCE {nm}: two runs")
    g = runs[0]
    want = W.head_backward(KS, 0, 0, D, out32, None, 1.0 / M)
    assert set(want) | {"dlogit"} == set(g)
    for nm, (w, b) in want.items():
        assert_bounded(g[nm], w, b, f"rowdot fused BCE M={M} {kind} {gkind} {nm}")
    # dlogit is the d that dbias sums: the gradient of the loss with respect to the logit, 0 outside the row's own column
    own = np.zeros(M, dtype=np.int64) if grp is None else np.where((grp < 0) | (grp >= n), 0, grp)
    o, t = out32.astype(np.float64), D["y"].astype(np.float64)
    d = np.zeros((M, n))
    oo = o[np.arange(M), own]
    d[np.arange(M), own] = (1.0 / M) * (oo - t) / np.maximum((1.0 - oo) * oo, 1e-12) * oo * (1.0 - oo)
    assert_bounded(g["dlogit"], d, 10 * I.U24 * np.abs(d), f"rowdot fused BCE M={M} {kind} {gkind} dlogit")      # cd = 7 + 3 roundings
    assert not g["dlogit"][d == 0].any()


def test_rowdot_fused_bce_argument_checks(cuda, lib):
    from cdcmdr_amd import _lib as L
    t, ws, loss = torch.full((16,), 0.5, device=cuda), torch.zeros(PARTS * 5, device=cuda), torch.zeros(1, device=cuda)
    dbl = torch.zeros(PARTS, dtype=torch.float64, device=cuda)
    y = torch.zeros(4, dtype=torch.int16, device=cuda)
    ro = torch.tensor([0, 4], dtype=torch.int32, device=cuda)

    def args(**kw):
        a = L.RowdotBwdArgs()
        a.n_groups, a.sigmoid, a.M, a.workspace = 1, 1, 4, ws.data_ptr()
        G = a.g[0]
        G.x, G.ldx, G.w, G.K, G.out, G.ld_out, G.dout, G.ld_dout = t.data_ptr(), 4, t.data_ptr(), 4, t.data_ptr(), 1, t.data_ptr(), 1
        a.bce_y_i16, a.bce_loss, a.bce_partial, a.bce_inv_count = y.data_ptr(), loss.data_ptr(), dbl.data_ptr(), 0.25
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.cdc_rowdot_bwd(C.byref(args(row_offsets=ro.data_ptr())), _stream()) == BADARG
    assert b"the fused BCE needs sigmoid outputs, dense rows" in lib.cdc_last_error()
    assert lib.cdc_rowdot_bwd(C.byref(args(sigmoid=0)), _stream()) == BADARG
    assert b"the fused BCE needs sigmoid outputs, dense rows" in lib.cdc_last_error()
    assert lib.cdc_rowdot_bwd(C.byref(args()), _stream()) == 0
