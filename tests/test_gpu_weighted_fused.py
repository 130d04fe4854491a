"""The fused launches with a loss-weight operand (`bce_weight` of cdc_tower_args, cdc_head_args and cdc_rowdot_bwd_args) straight
through the C-ABI.

Towers: tests/test_gpu_tower_direct.py's Launch with `a.bce_weight` set, against tests/tower_ref.py with its logit gradients
wrapped by tests/weighted_ref.py (tests/test_weighted_loss_cpu.py holds that wrapper to torch autograd).  Head and row-dot: the
pattern of the fused-BCE tests of tests/test_gpu_head.py, against weighted_ref.head_backward.

Bit equalities the contract states, asserted with assert_bits_equal on every output: all-ones weights are the NULL pointer; a
uniform weight 4 is the NULL pointer with 4 * inv_count (a power of two scales every operation exactly); cdc_tower_step is the two
launches; one rank through the six cdc_tower_dp phases is the two launches (the loss, another order of the same double sum, to its
float64 bound); the head's fused form is the WEIGHTED stand-alone launch followed by the d_out path; a tower all of whose rows
weigh 0 gets exactly zero gradients."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_head as H
import tower_ref as R
import weighted_ref as W
from helpers import PAD, SUM_FIG, U24, PadBuf, assert_bits_equal, assert_bounded, capped, nan_like
from test_gpu_tower_direct import DP_CASES, Launch, data, same_bits

pytestmark = pytest.mark.gpu
NAMES = ["rows2_bce", "rows65_bce", "rows129_bce", "rows257_bce", "h128_65", "nt1", "nt4", "bce_nogroup", "bce_outside", "bce_one", "extreme",
         "accwide_bce", "wide512", "resident256"]
_TWO = {}


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def launch(lib, dev, c, w, D=None, **kw):
    """a fresh Launch of the case with the row weights w (None: the pointer stays NULL)"""
    A = Launch(lib, dev, c, data(c) if D is None else D, **kw)
    if w is not None:
        A.a.bce_weight = A._k(torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev)).data_ptr()
    return A


def two(A):
    A.run("cdc_tower_fwd")
    f = A.forward()
    A.run("cdc_tower_bwd")
    return f, A.backward()


def weighted_two(lib, dev, c):
    """the two launches with the case's seeded weights: run once, shared by the tests of the case, never changed"""
    if c["name"] not in _TWO:
        _TWO[c["name"]] = two(launch(lib, dev, c, W.weights(c["name"], c["M"])))
    return _TWO[c["name"]]


# ------------------------------------------------------------------------------------------------------------------------
# towers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_weighted_towers_against_float64(cuda, lib, name, monkeypatch):
    c = R.by_name(name)
    D, w = data(c), W.weights(name, c["M"])
    f, b = weighted_two(lib, cuda, c)
    S = R.saved({**f, **b}, c)
    R.compare(f, R.ref_forward(c, D, S), f"{name} weighted fwd")
    monkeypatch.setattr(R, "logit_gradients", W.tower_logit_gradients(w))
    want = R.ref_backward(c, D, S)
    R.compare(b, want, f"{name} weighted bwd")
    assert {k for k, v in want.items() if isinstance(v, tuple)} == set(b)
    # one launch for both directions: the two launches' bits
    A = launch(lib, cuda, c, w).run("cdc_tower_step")
    same_bits(A.forward(), f, f"{name} weighted step, forward")
    same_bits(A.backward(), b, f"{name} weighted step, backward")


@pytest.mark.parametrize("name", NAMES)
def test_tower_weights_of_one_and_of_four_are_the_null_pointer(cuda, lib, name):
    c = R.by_name(name)
    M = c["M"]
    f0, b0 = two(launch(lib, cuda, c, None))
    f1, b1 = two(launch(lib, cuda, c, np.ones(M)))
    same_bits(f1, f0, f"{name} all-ones, forward")
    same_bits(b1, b0, f"{name} all-ones, backward")
    inv4 = 4.0 * R.inv_count(c)
    f4, b4 = two(launch(lib, cuda, c, np.full(M, 4.0)))
    fs, bs = two(launch(lib, cuda, c, None, inv_count=inv4))
    same_bits(f4, fs, f"{name} uniform 4, forward")
    same_bits(b4, bs, f"{name} uniform 4, backward")


@pytest.mark.parametrize("name", ["rows2_bce", "rows129_bce", "rows257_bce"])
def test_six_weighted_phases_on_one_rank_equal_the_two_launches(cuda, lib, name, monkeypatch):
    c = R.by_name(name)
    D, w = data(c), W.weights(name, c["M"])
    f, b = weighted_two(lib, cuda, c)
    A = launch(lib, cuda, c, w, dp=True)
    for phase in range(1, 7):
        A.run("cdc_tower_dp", phase)
    fd, bd = A.forward(), A.backward()
    same_bits(fd, f, f"{name} weighted dp, forward")
    same_bits(bd, b, f"{name} weighted dp, backward", skip=("loss",))
    monkeypatch.setattr(R, "logit_gradients", W.tower_logit_gradients(w))
    want = R.ref_backward(c, D, R.saved({**fd, **bd}, c))["loss"]
    assert_bounded(bd["loss"], want[0], want[1], f"{name} weighted dp loss")


DP_BCE = [c for c in DP_CASES if R.bce(c)]


@pytest.mark.parametrize("shares", [(128, 1), (65, 64)], ids=["128+1", "65+64"])
@pytest.mark.parametrize("c", DP_BCE, ids=[c["name"] for c in DP_BCE])
def test_two_simulated_ranks_against_the_weighted_global_batch(cuda, lib, c, shares, monkeypatch):
    """tests/test_gpu_tower_direct.py::test_two_simulated_ranks_against_the_global_batch with each rank holding the weights of its
    own rows"""
    D, w = data(c), W.weights(c["name"], c["M"])
    n = c["n_tower"]
    ranks, lo = [], 0
    for m in shares:
        rows = slice(lo, lo + m)
        Dk = {k: ([a[rows] if (k in ("x", "dx0")) else a for a in v] if isinstance(v, list) else v) for k, v in D.items()}
        for k in ("wx", "wdx0", "dout", "y", "group"):
            if Dk.get(k) is not None:
                Dk[k] = np.ascontiguousarray(D[k][rows])
        ranks.append(launch(lib, cuda, dict(c, M=m), np.ascontiguousarray(w[rows]), D=Dk, dp=True, inv_count=R.inv_count(c)))
        lo += m
    for phase in range(1, 7):
        for A in ranks:
            A.run("cdc_tower_dp", phase)
        e = {1: 0, 2: 1, 4: 2, 5: 3}.get(phase)
        if e is not None:                                            # the all-reduce of the exchange buffer
            total = ranks[0].ex[e] + ranks[1].ex[e]
            for A in ranks:
                A.ex[e].copy_(total)
            assert total[-n:].tolist() == [float(c["M"])] * n
    F, Bk = [A.forward() for A in ranks], [A.backward() for A in ranks]
    got, local = {}, {}
    for k in list(F[0]) + list(Bk[0]):
        u, v = (F[0][k], F[1][k]) if k in F[0] else (Bk[0][k], Bk[1][k])
        if k.startswith(("mean", "inv", "rm", "rv", "nbt")):
            if k.startswith("nbt"):
                assert u == v
            else:
                assert_bits_equal(u, v, f"{k} on the two ranks")
            got[k] = u
        elif k.startswith(("dgamma", "dbeta", "dwo", "dbo", "wide_dw", "wide_dbias", "loss")):
            got[k], local[k] = u.astype(np.float64) + v.astype(np.float64), np.abs(u).astype(np.float64) + np.abs(v)
        else:
            got[k] = np.concatenate([u, v], 0)
    S = R.saved(got, c)
    R.compare(got, R.ref_forward(c, D, S), f"{c['name']} {shares} weighted fwd")
    monkeypatch.setattr(R, "logit_gradients", W.tower_logit_gradients(w))
    want = R.ref_backward(c, D, S)
    for k, v in want.items():
        if isinstance(v, tuple):
            bound = v[1] if k not in local else capped(v[1] + U24 * local[k], v[0], SUM_FIG)      # each rank rounds its local sum
            assert_bounded(got[k], v[0], bound, f"{c['name']} {shares} weighted bwd {k}")


def test_a_tower_whose_rows_all_weigh_zero_gets_exactly_zero_gradients(cuda, lib):
    """what bce_one asserts without weights: tower 1's workgroups see nothing but zero logit gradients"""
    c = R.by_name("rows129_bce")
    D = data(c)
    w = W.weights("zero_tower", c["M"])
    own = R.own_tower(c, D)
    w[own == 1] = 0.0
    assert (own == 1).sum() > 10 and (w[own != 1] > 0).sum() > 10
    _, b = two(launch(lib, cuda, c, w))
    for k in ("dwo", "dbo", "dgamma1", "dgamma2", "dbeta1", "dbeta2", "dx", "dzh1", "dzh2"):
        assert not b[f"{k}_1"].any(), f"{k}_1"
        assert b[f"{k}_0"].any(), f"{k}_0"


# ------------------------------------------------------------------------------------------------------------------------
# the tower head
# ------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def head_spec(M, nt):
    K = (33,) if nt == 1 else (16, 40, 64)
    return dict(name=f"w{M}x{nt}", K=K, wide=26, M=M, n_add=1, bias=True, sigmoid=1, acc_dx=(0,) * nt, acc_wide=0, acc_add=(0,),
                wide_out=False, wide_bias=True, no_dx=(), no_dw=(), no_dadd=(), ld_dout_extra=0)


def head_backward(cuda, s, D, out32, bce, w=None, inv=None):
    A = H.Launch(cuda, s, D, out32=out32, bce=bce)
    if w is not None:
        A.a.bce_weight = A._k(torch.from_numpy(np.asarray(w, dtype=np.float32)).to(cuda)).data_ptr()
    if inv is not None:
        A.a.bce_inv_count = inv
    return A.backward()


@pytest.mark.parametrize("gkind", ["none", "outside"])
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("M", [2, 65, 257])
def test_head_weighted_fused_bce(cuda, M, nt, kind, gkind):
    from cdcmdr_amd import _lib as L
    lib = L.load()
    s = head_spec(M, nt)
    bce = (kind, gkind)
    D = H.make_data(s, bce)
    w = W.weights(s["name"], M)
    out32 = H.Launch(cuda, s, D).forward()["out"]
    assert (out32 == 1).any()
    g = head_backward(cuda, s, D, out32, bce, w)
    want = W.head_backward(s["K"], s["wide"], s["n_add"], D, out32, w, 1.0 / M)
    assert set(want) == set(g)
    H.compare(g, want, f"head {s['name']} {kind} {gkind} weighted")
    for t in range(nt):
        assert not g[f"dx{t}"][w == 0].any(), "a row of weight 0 has a gradient"
    # all-ones weights: the NULL pointer; a uniform 4: the NULL pointer with 4 * inv_count
    plain, ones = head_backward(cuda, s, D, out32, bce), head_backward(cuda, s, D, out32, bce, np.ones(M))
    four, scaled = head_backward(cuda, s, D, out32, bce, np.full(M, 4.0)), head_backward(cuda, s, D, out32, bce, inv=4.0 / M)
    for k in plain:
        assert_bits_equal(ones[k], plain[k], f"head {s['name']} {k}: all-ones weights")
        assert_bits_equal(four[k], scaled[k], f"head {s['name']} {k}: uniform weight 4")
    # the two-launch form: the WEIGHTED stand-alone launch on `out`, its dp as d_out of the head's backward
    p, dp = PadBuf(cuda, out32), PadBuf(cuda, nan_like(M, nt), out=True)
    y, wt = torch.from_numpy(D["y"]).to(cuda), torch.from_numpy(w).to(cuda)
    grp = None if D["group"] is None else torch.from_numpy(D["group"]).to(cuda)
    loss = torch.full((1,), float("nan"), device=cuda)
    L.check(lib.cdc_bce_weighted_fwd_bwd(p.ptr, p.ld, None if grp is None else grp.data_ptr(), y.data_ptr() if kind == "i16" else None,
                                         y.data_ptr() if kind == "f32" else None, wt.data_ptr(), loss.data_ptr(), dp.ptr, dp.ld, M, nt,
                                         1.0 / M, _stream()), "weighted bce")
    g3 = H.Launch(cuda, dict(s, ld_dout_extra=PAD), dict(D, dout=dp.read("dp")), out32=out32).backward()
    assert_bits_equal(g["loss"], loss.cpu().numpy(), f"head {s['name']}: fused loss vs cdc_bce_weighted_fwd_bwd")
    for k in g3:
        assert_bits_equal(g[k], g3[k], f"head {s['name']} {k}: fused vs cdc_bce_weighted_fwd_bwd + d_out")


# ------------------------------------------------------------------------------------------------------------------------
# the row-dot backward: the launch's groups are the columns of one prediction matrix
# ------------------------------------------------------------------------------------------------------------------------
PARTS = 256


def rowdot_backward(cuda, K, D, out32, w=None, inv=None):
    from cdcmdr_amd import _lib as L
    lib = L.load()
    M, nt = out32.shape
    a = L.RowdotBwdArgs()
    keep = []
    k = lambda b: keep.append(b) or b
    out = k(PadBuf(cuda, out32))
    a.n_groups, a.sigmoid, a.M = nt, 1, M
    res = {}
    for t, Kt in enumerate(K):
        G = a.g[t]
        x, wt = k(PadBuf(cuda, D["x"][t])), k(PadBuf(cuda, D["w"][t]))
        G.out, G.ld_out = out.ptr + 4 * t, out.ld
        G.x, G.ldx, G.w, G.K = x.ptr, x.ld, wt.ptr, Kt
        res[f"dx{t}"], res[f"dw{t}"], res[f"dbias{t}"] = (PadBuf(cuda, nan_like(M, Kt), out=True), PadBuf(cuda, nan_like(1, Kt), out=True),
                                                         PadBuf(cuda, nan_like(1, 1), out=True))
        G.dx, G.lddx, G.dw, G.dbias = res[f"dx{t}"].ptr, res[f"dx{t}"].ld, res[f"dw{t}"].ptr, res[f"dbias{t}"].ptr
    y = k(torch.from_numpy(D["y"]).to(cuda))
    if D["y"].dtype == np.int16:
        a.bce_y_i16 = y.data_ptr()
    else:
        a.bce_y_f32 = y.data_ptr()
    if D["group"] is not None:
        a.bce_group = k(torch.from_numpy(D["group"]).to(cuda)).data_ptr()
    loss = torch.full((1,), float("nan"), device=cuda)
    a.bce_loss = loss.data_ptr()
    a.bce_partial = k(torch.full((nt * PARTS,), float("nan"), dtype=torch.float64, device=cuda)).data_ptr()
    a.bce_inv_count = 1.0 / M if inv is None else inv
    if w is not None:
        a.bce_weight = k(torch.from_numpy(np.asarray(w, dtype=np.float32)).to(cuda)).data_ptr()
    a.workspace = k(torch.full((nt * PARTS * (max(K) + 1),), float("nan"), device=cuda)).data_ptr()
    L.check(lib.cdc_rowdot_bwd(C.byref(a), _stream()), "cdc_rowdot_bwd")
    got = {name: b.read(name) for name, b in res.items()}
    got["loss"] = loss.cpu().numpy()
    return got


@pytest.mark.parametrize("gkind", ["none", "outside"])
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("M", [2, 65, 257])
def test_rowdot_weighted_fused_bce(cuda, M, nt, kind, gkind):
    s = head_spec(M, nt)
    D = H.make_data(s, (kind, gkind))
    w = W.weights(s["name"] + "rowdot", M)
    rng = np.random.default_rng(M + nt)
    out32 = rng.uniform(0.02, 0.98, size=(M, nt)).astype(np.float32)
    out32[0], out32[1] = 1.0, 0.0                                     # both clamps of the loss and the 1e-12 floor
    g = rowdot_backward(cuda, s["K"], D, out32, w)
    want = W.head_backward(s["K"], 0, 0, D, out32, w, 1.0 / M)
    assert set(want) == set(g)
    H.compare(g, want, f"rowdot {s['name']} {kind} {gkind} weighted")
    for t in range(nt):
        assert not g[f"dx{t}"][w == 0].any(), "a row of weight 0 has a gradient"
    plain, ones = rowdot_backward(cuda, s["K"], D, out32), rowdot_backward(cuda, s["K"], D, out32, np.ones(M))
    four, scaled = rowdot_backward(cuda, s["K"], D, out32, np.full(M, 4.0)), rowdot_backward(cuda, s["K"], D, out32, inv=4.0 / M)
    for k in plain:
        assert_bits_equal(ones[k], plain[k], f"rowdot {s['name']} {k}: all-ones weights")
        assert_bits_equal(four[k], scaled[k], f"rowdot {s['name']} {k}: uniform weight 4")
