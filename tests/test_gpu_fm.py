"""cdc_fm_fwd / cdc_fm_bwd (csrc/rowops.hip) straight through the C-ABI against float64 (tests/interaction_ref.py): padded
lde / ldde, out and dout as column 1 of a three-wide buffer (ldo = ldd = 3), the backward as a plain store (target pre-filled with
NaN) and as an accumulate (random values); D below, at and above a wave's 64 lanes (a lane's second and third trip), row counts
that are no multiple of the four waves of a workgroup, one field (the exact result is 0)."""
import ctypes as C

import numpy as np
import pytest
import torch

import interaction_ref as I
from helpers import OUT_SENTINEL, PadBuf, assert_bounded, nan_like

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 3, 16), (7, 26, 16), (3, 2, 65), (6, 4, 130)]
BADARG = -1


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _col1(cuda, values, out=False):
    """[B] values as column 1 of a [B, 3] buffer: NaN (input) or the sentinel (output) in columns 0 and 2"""
    B = len(values)
    host = np.full((B, 3), OUT_SENTINEL if out else np.nan, dtype=np.float32)
    host[:, 1] = values
    return torch.from_numpy(host).to(cuda)


@pytest.mark.parametrize("B,F,D", SHAPES)
def test_fm_against_float64(cuda, lib, B, F, D):
    from cdcmdr_amd import _lib as L
    rng = np.random.default_rng(B * 1000 + F * 10 + D)
    e = rng.standard_normal((B, F * D)).astype(np.float32)
    dout, old = rng.standard_normal(B).astype(np.float32), rng.standard_normal((B, F * D)).astype(np.float32)
    E = PadBuf(cuda, e)
    out = _col1(cuda, np.full(B, np.nan, dtype=np.float32), out=True)
    L.check(lib.cdc_fm_fwd(E.ptr, E.ld, out.data_ptr() + 4, 3, B, F, D, _stream()), "cdc_fm_fwd")
    o = out.cpu().numpy()
    assert (o[:, [0, 2]] == np.float32(OUT_SENTINEL)).all(), "fm_fwd wrote beside its column"
    want, bound = I.fm_forward(e, F, D)
    assert_bounded(o[:, 1], want, bound, f"fm_fwd ({B}, {F}, {D})")
    if F == 1:
        assert (bound > 0).all()                                               # exactly 0, and room for one rounding of v^2
    DO = _col1(cuda, dout)
    for acc in (0, 1):
        de = PadBuf(cuda, old if acc else nan_like(B, F * D), out=True)
        L.check(lib.cdc_fm_bwd(E.ptr, E.ld, DO.data_ptr() + 4, 3, de.ptr, de.ld, B, F, D, acc, _stream()), "cdc_fm_bwd")
        w, b = I.fm_backward(e, dout, F, D, old if acc else None)
        assert_bounded(de.read("fm de"), w, b, f"fm_bwd ({B}, {F}, {D}) accumulate={acc}")


def test_fm_empty_batch_and_argument_checks(cuda, lib):
    t = torch.full((64,), float("nan"), device=cuda)
    p, s = t.data_ptr(), _stream()
    assert lib.cdc_fm_fwd(p, 8, p, 1, 0, 2, 4, s) == 0 and lib.cdc_fm_bwd(p, 8, p, 1, p, 8, 0, 2, 4, 0, s) == 0
    assert bool(torch.isnan(t).all())
    assert lib.cdc_fm_fwd(p, 7, p, 1, 1, 2, 4, s) == BADARG and b"fm_fwd: bad argument" in lib.cdc_last_error()       # lde < F D
    assert lib.cdc_fm_fwd(p, 8, p, 0, 1, 2, 4, s) == BADARG                                                          # ldo < 1
    assert lib.cdc_fm_bwd(p, 8, p, 1, p, 7, 1, 2, 4, 0, s) == BADARG and b"fm_bwd: bad argument" in lib.cdc_last_error()
