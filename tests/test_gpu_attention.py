"""cdc_attn_fwd / cdc_attn_bwd (csrc/attention.hip) straight through the C-ABI against float64 (tests/interaction_ref.py, held to
torch autograd by tests/test_interaction_ref_cpu.py), with the conventions of tests/test_gpu_head.py: every leading dimension
padded (NaN in input padding, a sentinel that must survive in output padding), store targets pre-filled with NaN, derived bounds
capped by the suite's present figures.  Every head dim of the contract, F up to 64, the LDS sizes on both sides of 64 KB and the
contract's largest shapes, which need fewer than four waves per workgroup; dropout with the step counter on the device, its mask
regenerated on the host; and the bits of the reference's geometry, which the choice of the workgroup size must not move."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import interaction_ref as I
from helpers import OUT_SENTINEL, PadBuf, assert_bits_equal, assert_bounded, nan_like

pytestmark = pytest.mark.gpu

# (B, F, A, H)
SHAPES = [(1, 1, 4, 1), (5, 6, 16, 2), (3, 26, 48, 3), (7, 26, 64, 2), (2, 33, 64, 1), (2, 63, 8, 1), (3, 64, 16, 4),
          (2, 64, 64, 2), (2, 48, 64, 1), (1, 64, 64, 1)]       # the last three: more than 160 KB of LDS with four waves
SEED, STEP, P = 0x5EED0A77E4710D5, 3, 0.5
BADARG = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_7_26_64_2_bits.json")
GUARD = 5


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def data(B, F, A, H):
    rng = np.random.default_rng(B * 100000 + F * 1000 + A * 10 + H)
    return rng.standard_normal((B * F, 3 * A)).astype(np.float32), rng.standard_normal((B * F, A)).astype(np.float32)


def _step_ptr(cuda, step, keep):
    if step is None:
        return None
    keep.append(torch.tensor([step], dtype=torch.int32, device=cuda))
    return keep[-1].data_ptr()


def forward(cuda, lib, qkv, shape, p=0.0, step=None, with_probs=True):
    """(out [B F, A], probs [B, H, F, F] or None) of one launch; checks the padding and the guard elements behind probs"""
    from cdcmdr_amd import _lib as L
    B, F, A, H = shape
    keep = []
    Q, O = PadBuf(cuda, qkv), PadBuf(cuda, nan_like(B * F, A), out=True)
    n = B * H * F * F
    Pb = torch.full((n + GUARD,), float("nan"), device=cuda)
    Pb[n:] = OUT_SENTINEL
    L.check(lib.cdc_attn_fwd(Q.ptr, Q.ld, O.ptr, O.ld, Pb.data_ptr() if with_probs else None, B, F, A, H, p, SEED, _step_ptr(cuda, step, keep),
                             _stream()), "cdc_attn_fwd")
    pr = Pb.cpu().numpy()
    assert (pr[n:] == np.float32(OUT_SENTINEL)).all(), "attn_fwd wrote past probs"
    if not with_probs:
        assert np.isnan(pr[:n]).all(), "attn_fwd wrote probs through a NULL pointer's neighbour"
    return O.read("attention out"), (pr[:n].reshape(B, H, F, F).copy() if with_probs else None)


def backward(cuda, lib, qkv, probs, dout, shape, p=0.0, step=None):
    """dqkv [B F, 3A], pre-filled with NaN: the backward writes every column"""
    from cdcmdr_amd import _lib as L
    B, F, A, H = shape
    keep = []
    Q, DO, DQ = PadBuf(cuda, qkv), PadBuf(cuda, dout), PadBuf(cuda, nan_like(B * F, 3 * A), out=True)
    Pb = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).to(cuda)
    L.check(lib.cdc_attn_bwd(Q.ptr, Q.ld, Pb.data_ptr(), DO.ptr, DO.ld, DQ.ptr, DQ.ld, B, F, A, H, p, SEED, _step_ptr(cuda, step, keep),
                             _stream()), "cdc_attn_bwd")
    return DQ.read("dqkv")


def _compare_backward(g, want, A, what):
    for i, nm in enumerate(("dq", "dk", "dv")):
        assert_bounded(g[:, i * A:(i + 1) * A], want[nm][0], want[nm][1], f"{what} {nm}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_against_float64(cuda, lib, shape):
    B, F, A, H = shape
    qkv, dout = data(*shape)
    keep = np.ones((B, H, F, F), dtype=bool)
    out, probs = forward(cuda, lib, qkv, shape)
    want = I.attn_forward(qkv, B, F, A, H, keep, 0.0)
    assert_bounded(probs, want["probs"][0], want["probs"][1], f"attn {shape} probs")
    assert_bounded(out, want["out"][0], want["out"][1], f"attn {shape} out")
    g = backward(cuda, lib, qkv, probs, dout, shape)
    _compare_backward(g, I.attn_backward(qkv, probs, dout, B, F, A, H, keep, 0.0), A, f"attn {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_dropout_with_device_step(cuda, lib, shape):
    B, F, A, H = shape
    qkv, dout = data(*shape)
    keep = I.attn_keep_mask(SEED, STEP, B, H, F, P)
    out, probs = forward(cuda, lib, qkv, shape, P, STEP)
    want = I.attn_forward(qkv, B, F, A, H, keep, P)
    assert_bounded(probs, want["probs"][0], want["probs"][1], f"attn {shape} p={P} probs: the softmax before dropout")
    assert_bounded(out, want["out"][0], want["out"][1], f"attn {shape} p={P} out")
    plain_out, plain_probs = forward(cuda, lib, qkv, shape)
    assert_bits_equal(probs, plain_probs, f"attn {shape}: the saved probabilities do not depend on dropout")
    g = backward(cuda, lib, qkv, probs, dout, shape, P, STEP)
    _compare_backward(g, I.attn_backward(qkv, probs, dout, B, F, A, H, keep, P), A, f"attn {shape} p={P}")
    # the step counter moves the mask; the NULL pointer is step 0
    out4, _ = forward(cuda, lib, qkv, shape, P, STEP + 1)
    if F > 1:
        assert not np.array_equal(out4, out), "another step, the same mask"
        assert not np.array_equal(out, plain_out)
    out_null, _ = forward(cuda, lib, qkv, shape, P, None)
    out_zero, _ = forward(cuda, lib, qkv, shape, P, 0)
    assert_bits_equal(out_null, out_zero, f"attn {shape}: seed_offset_dev NULL against step 0")
    want0 = I.attn_forward(qkv, B, F, A, H, I.attn_keep_mask(SEED, None, B, H, F, P), P)
    assert_bounded(out_null, want0["out"][0], want0["out"][1], f"attn {shape} p={P} out, NULL step")
    g_null = backward(cuda, lib, qkv, probs, dout, shape, P, None)
    assert_bits_equal(g_null, backward(cuda, lib, qkv, probs, dout, shape, P, 0), f"attn {shape}: backward, NULL against step 0")


def test_attention_null_probs_and_empty_batch(cuda, lib):
    shape = (5, 6, 16, 2)
    B, F, A, H = shape
    qkv, dout = data(*shape)
    for p, step in ((0.0, None), (P, STEP)):
        a, _ = forward(cuda, lib, qkv, shape, p, step)
        b, none = forward(cuda, lib, qkv, shape, p, step, with_probs=False)
        assert none is None
        assert_bits_equal(a, b, "attn_fwd: probs NULL")
    # B = 0: returns 0 and writes nothing
    Q, O, DQ = PadBuf(cuda, qkv), PadBuf(cuda, nan_like(B * F, A), out=True), PadBuf(cuda, nan_like(B * F, 3 * A), out=True)
    DO = PadBuf(cuda, dout)
    Pb = torch.full((B * H * F * F,), float("nan"), device=cuda)
    assert lib.cdc_attn_fwd(Q.ptr, Q.ld, O.ptr, O.ld, Pb.data_ptr(), 0, F, A, H, 0.0, SEED, None, _stream()) == 0
    assert lib.cdc_attn_bwd(Q.ptr, Q.ld, Pb.data_ptr(), DO.ptr, DO.ld, DQ.ptr, DQ.ld, 0, F, A, H, 0.0, SEED, None, _stream()) == 0
    assert np.isnan(O.read("out")).all() and np.isnan(DQ.read("dqkv")).all() and bool(torch.isnan(Pb).all())


def test_attention_argument_checks(cuda, lib):
    t = torch.zeros(65 * 3 * 64 + 64, device=cuda)
    p = t.data_ptr()
    s = _stream()
    # (F, A, H, drop_p, ld): F = 65; A % H != 0; dh = 12; p = 1; ld < 3A
    for F, A, H, dp, ld in ((65, 8, 1, 0.0, 24), (4, 10, 4, 0.0, 30), (4, 24, 2, 0.0, 72), (4, 8, 1, 1.0, 24), (4, 8, 1, 0.0, 23)):
        assert lib.cdc_attn_fwd(p, ld, p, A, p, 1, F, A, H, dp, 1, None, s) == BADARG, (F, A, H, dp, ld)
        assert b"attn_fwd: bad argument" in lib.cdc_last_error()
        assert lib.cdc_attn_bwd(p, ld, p, p, A, p, 3 * A, 1, F, A, H, dp, 1, None, s) == BADARG, (F, A, H, dp, ld)
        assert b"attn_bwd: bad argument" in lib.cdc_last_error()
    assert lib.cdc_attn_fwd(p, 24, p, 7, p, 1, 4, 8, 1, 0.0, 1, None, s) == BADARG                  # ldo < A
    assert lib.cdc_attn_bwd(p, 24, p, p, 7, p, 24, 1, 4, 8, 1, 0.0, 1, None, s) == BADARG           # lddo < A
    assert lib.cdc_attn_bwd(p, 24, p, p, 8, p, 23, 1, 4, 8, 1, 0.0, 1, None, s) == BADARG           # lddq < 3A


def test_attention_accepts_every_shape_of_the_contract(cuda, lib):
    """include/cdcmdr.h: F <= 64, dh in {4, 8, 16, 32, 64} — both launches take every such shape (three pairs: with one, two or four
    waves per workgroup some workgroup has a dead wave) and the backward writes every element of dqkv."""
    B, H = 3, 1
    qkv = torch.randn(B * 64 * 3 * 64, device=cuda)
    dout = torch.randn(B * 64 * 64, device=cuda)
    out, probs = torch.empty(B * 64 * 64, device=cuda), torch.empty(B * 64 * 64, device=cuda)
    s = _stream()
    for dh in (4, 8, 16, 32, 64):
        for F in range(1, 65):
            dq = torch.full((B * F * 3 * dh,), float("nan"), device=cuda)
            assert lib.cdc_attn_fwd(qkv.data_ptr(), 3 * dh, out.data_ptr(), dh, probs.data_ptr(), B, F, dh, H, 0.0, 1, None, s) == 0, \
                (F, dh, lib.cdc_last_error())
            assert lib.cdc_attn_bwd(qkv.data_ptr(), 3 * dh, probs.data_ptr(), dout.data_ptr(), dh, dq.data_ptr(), 3 * dh, B, F, dh, H, 0.0, 1,
                                    None, s) == 0, (F, dh, lib.cdc_last_error())
            assert not bool(torch.isnan(dq).any()), (F, dh)


def golden_bits(cuda, lib):
    """sha256 of the outputs' bytes at the reference's geometry, without dropout and with it"""
    shape = (7, 26, 64, 2)
    qkv, dout = data(*shape)
    R = {}
    for tag, p, step in (("plain", 0.0, None), ("dropout", P, STEP)):
        out, probs = forward(cuda, lib, qkv, shape, p, step)
        g = backward(cuda, lib, qkv, probs, dout, shape, p, step)
        for nm, a in (("out", out), ("probs", probs), ("dqkv", g)):
            R[f"{tag}_{nm}"] = hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()
    return R


def test_attention_bits_at_the_reference_geometry(cuda, lib):
    """Every wave is independent and the dropout index does not depend on a wave's place in its workgroup, so the number of waves
    per workgroup moves no bit: (7, 26, 64, 2) against the hashes recorded from the build that always ran four waves."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = golden_bits(cuda, lib)
    assert set(got) == set(want["sha256"])
    for k, v in got.items():
        assert v == want["sha256"][k], f"attention (7, 26, 64, 2) {k}: bits moved"
