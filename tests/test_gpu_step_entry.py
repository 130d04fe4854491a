"""The launches a training step begins with, straight through the C-ABI; every comparison is exact.  cdc_embed_gather_fwd_h (the
gather training calls, with and without its bf16 shadow, on the 16-byte and the scalar path, past its grid cap), cdc_embed_index,
cdc_stage_batch / cdc_stage_batch_next and the small utilities of csrc/misc.hip (cdc_fill_f32, cdc_fill_f64, cdc_add_inplace,
cdc_step_increment).  Every destination is pre-filled with a value no launch writes and followed by guard elements that must come
back unchanged; ids include a negative sum, a sum that wraps in int32, a row just past the table and a negative id whose sum lands
inside the table (taken like any other: the reference adds in int32)."""
import ctypes as C

import numpy as np
import pytest
import torch

from bn_ref import bf16_bits
from helpers import OUT_SENTINEL, PadBuf, PadBufH, assert_bits_equal, nan_like

pytestmark = pytest.mark.gpu

BADARG = -1
GUARD = 7
I32_FILL, I32_GUARD = -7, -99


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    from cdcmdr_amd import _lib as L
    L.check(getattr(lib, name)(*args, _stream()), name)


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class Guarded:
    """n elements pre-filled with `fill`, then GUARD elements of `guard`; read() checks the guard and returns the n elements"""

    def __init__(self, dev, n, dtype, fill, guard):
        host = np.full(n + GUARD, fill, dtype=dtype)
        host[n:] = guard
        self.n, self.host0 = n, host
        self.t = torch.from_numpy(host.copy()).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self, what):
        h = self.t.cpu().numpy()
        assert h[self.n:].tobytes() == self.host0[self.n:].tobytes(), f"{what}: written past its end"
        return h[:self.n].copy()

    def untouched(self, what):
        assert self.t.cpu().numpy().tobytes() == self.host0.tobytes(), f"{what}: written"


# ------------------------------------------------------------------------------------------------------------------------
# the gather and the row indices
# ------------------------------------------------------------------------------------------------------------------------
def make_ids(rng, B, F, with_bad=True):
    """ids [B, F], offsets [F], R, and the float64-free expectation: idx [B, F] (-1 for a row outside the table) and the flag"""
    vocab = rng.integers(3, 50, size=F)
    offsets = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int32)
    R = int(vocab.sum())
    ids = np.stack([rng.integers(0, v, size=B) for v in vocab], axis=1).astype(np.int32)
    n = B * F
    flat = ids.reshape(-1)
    if with_bad and n >= 3:
        for i, pos in enumerate(sorted({1, n // 2, n - 2} if n >= 8 else {1})):
            f = pos % F
            if i % 3 == 0:
                flat[pos] = -int(offsets[f]) - 5                                # the sum is -5
            elif i % 3 == 1:
                flat[pos] = 2 ** 31 - 1 if f > 0 else -7                        # the int32 sum wraps to a negative row
            else:
                flat[pos] = R - int(offsets[f])                                 # the first row past the table
        if n >= 8 and F > 1:
            flat[F + 1] = -1                                                    # field 1: row offsets[1] - 1, a row of field 0
    row = (flat.astype(np.uint32) + np.tile(offsets, B).astype(np.uint32)).astype(np.uint32).view(np.int32)
    ok = (row >= 0) & (row.astype(np.int64) < R)
    idx = np.where(ok, row, -1).astype(np.int32)
    flag = int(np.max(np.nonzero(~ok)[0]) + 1) if (~ok).any() else 0
    return ids, offsets, R, idx.reshape(B, F), flag


def _ld_h(F, D):
    """F D + 8 columns, rounded up to the multiple of four elements the launch requires of a shadow's row stride"""
    return F * D + 8 + (-(F * D)) % 4


GATHER = [(1, 3, 16, 0), (33, 5, 3, 0), (64, 7, 6, 0), (64, 7, 8, 1), (4100, 26, 40, 0)]


@pytest.mark.parametrize("shadow", [False, True], ids=["fp32", "shadow"])
@pytest.mark.parametrize("B,F,D,shift", GATHER)
def test_embed_gather_fwd_h(cuda, lib, B, F, D, shift, shadow):
    """shift = 1: the table starts one float past a 16-byte boundary, so D % 4 == 0 still takes the scalar path.  (4100, 26, 40):
    1 066 000 chunks of four floats, past the 4096 x 256 grid."""
    rng = np.random.default_rng(B * 1000 + F * 10 + D)
    ids, offsets, R, idx, flag = make_ids(rng, B, F)
    assert flag > 0 or B * F < 3
    table = rng.standard_normal((R, D)).astype(np.float32)
    T = _dev(cuda, np.concatenate([np.full(shift, np.nan, np.float32), table.reshape(-1)]))
    assert (T.data_ptr() + 4 * shift) % 16 == (4 * shift) % 16
    want = np.where((idx >= 0)[:, :, None], table[np.where(idx >= 0, idx, 0)], np.float32(0)).reshape(B, F * D)
    out = Guarded(cuda, B * F * D, np.float32, np.nan, OUT_SENTINEL)
    idx_out = Guarded(cuda, B * F, np.int32, I32_FILL, I32_GUARD)
    err = Guarded(cuda, 1, np.int32, 0, I32_GUARD)
    H = PadBufH(cuda, nan_like(B, F * D), out=True, pad=_ld_h(F, D) - F * D, extra_rows=1) if shadow else None
    d_ids, d_off = _dev(cuda, ids), _dev(cuda, offsets)
    call(lib, "cdc_embed_gather_fwd_h", d_ids.data_ptr(), d_off.data_ptr(), T.data_ptr() + 4 * shift, out.ptr,
         H.ptr if H else None, H.ld if H else 0, idx_out.ptr, err.ptr, B, F, D, R)
    got = out.read("gather out").reshape(B, F * D)
    assert_bits_equal(got, want, f"gather ({B}, {F}, {D}) out")
    assert np.array_equal(idx_out.read("gather idx").reshape(B, F), idx)
    assert int(err.read("gather flag")[0]) == flag
    if B * F >= 3:
        bad = (idx < 0)
        assert bad.any() and not got.reshape(B, F, D)[bad].any(), "a row outside the table gathers zeros"
    if shadow:
        hv = H.read("gather shadow")
        assert np.array_equal(bf16_bits(hv), bf16_bits(got)), f"gather ({B}, {F}, {D}) shadow: bf16 of the fp32 output"
    # idx_out and err_flag are optional
    out2 = Guarded(cuda, B * F * D, np.float32, np.nan, OUT_SENTINEL)
    call(lib, "cdc_embed_gather_fwd_h", d_ids.data_ptr(), d_off.data_ptr(), T.data_ptr() + 4 * shift, out2.ptr, None, 0, None, None, B, F, D, R)
    assert_bits_equal(out2.read("gather out").reshape(B, F * D), want, "gather without idx_out and err_flag")


def test_embed_gather_fwd_h_rejects_malformed_shadow(cuda, lib):
    t = torch.zeros(64, device=cuda)
    i = torch.zeros(8, dtype=torch.int32, device=cuda)
    p, q, s = t.data_ptr(), i.data_ptr(), _stream()
    for ld in (15, 18):                                                          # below F D = 16; not a multiple of 4
        assert lib.cdc_embed_gather_fwd_h(q, q, p, p, p, ld, None, None, 1, 2, 8, 4, s) == BADARG, ld
        assert b"malformed bf16 shadow" in lib.cdc_last_error()
    assert lib.cdc_embed_gather_fwd_h(q, q, p, p, p + 2, 16, None, None, 1, 2, 8, 4, s) == BADARG   # the shadow not 8-byte aligned
    assert lib.cdc_embed_gather_fwd_h(q, q, p, p, p + 32 * 4, 16, None, None, 0, 2, 8, 4, s) == 0   # B = 0: nothing to do
    assert not bool(t.any())


@pytest.mark.parametrize("B,F", [(1, 3), (33, 5), (64, 7), (40330, 26)])
def test_embed_index(cuda, lib, B, F):
    """(40330, 26): 1 048 580 positions, past the 4096 x 256 grid"""
    rng = np.random.default_rng(B + F)
    ids, offsets, R, idx, flag = make_ids(rng, B, F)
    d_ids, d_off = _dev(cuda, ids), _dev(cuda, offsets)
    for start in (0, B * F + 1000):                                              # the flag is a maximum: a larger value stays
        idx_out = Guarded(cuda, B * F, np.int32, I32_FILL, I32_GUARD)
        err = Guarded(cuda, 1, np.int32, start, I32_GUARD)
        call(lib, "cdc_embed_index", d_ids.data_ptr(), d_off.data_ptr(), idx_out.ptr, err.ptr, B, F, R)
        assert np.array_equal(idx_out.read("embed_index idx").reshape(B, F), idx)
        assert int(err.read("embed_index flag")[0]) == max(start, flag)
    idx_out = Guarded(cuda, B * F, np.int32, I32_FILL, I32_GUARD)
    call(lib, "cdc_embed_index", d_ids.data_ptr(), d_off.data_ptr(), idx_out.ptr, None, B, F, R)
    assert np.array_equal(idx_out.read("embed_index idx, no flag").reshape(B, F), idx)
    # clean ids leave the flag alone
    ids, offsets, R, idx, flag = make_ids(rng, B, F, with_bad=False)
    assert flag == 0 and (idx >= 0).all()
    idx_out, err = Guarded(cuda, B * F, np.int32, I32_FILL, I32_GUARD), Guarded(cuda, 1, np.int32, 0, I32_GUARD)
    d_ids, d_off = _dev(cuda, ids), _dev(cuda, offsets)
    call(lib, "cdc_embed_index", d_ids.data_ptr(), d_off.data_ptr(), idx_out.ptr, err.ptr, B, F, R)
    assert np.array_equal(idx_out.read("embed_index idx").reshape(B, F), idx) and int(err.read("flag")[0]) == 0


# ------------------------------------------------------------------------------------------------------------------------
# staging a batch
# ------------------------------------------------------------------------------------------------------------------------
# group, field_dims, the flag's start above every position, next_ids, step_dev (with n_acc = 2)
STAGE = [dict(group=1, fd=1, big=0, nxt=1, step=1), dict(group=0, fd=0, big=0, nxt=0, step=0), dict(group=1, fd=1, big=1, nxt=0, step=1),
         dict(group=0, fd=1, big=0, nxt=1, step=0)]


@pytest.mark.parametrize("v", range(len(STAGE)))
@pytest.mark.parametrize("B,F", [(1, 1), (300, 7), (20200, 26)])
def test_stage_batch_and_stage_batch_next(cuda, lib, B, F, v):
    """(20200, 26): 525 200 ids, past the 2048 x 256 grid"""
    c = STAGE[v]
    rng = np.random.default_rng(B + F + v)
    n = B * F
    fd = rng.integers(3, 50, size=F).astype(np.int32)
    ids = np.stack([rng.integers(0, d, size=B) for d in fd], axis=1).astype(np.int32)
    flat = ids.reshape(-1)
    for i, pos in enumerate(sorted({0, n // 3, n - 1})):
        flat[pos] = (-1, int(fd[pos % F]), 2 ** 31 - 1)[i % 3]                   # below 0, the first id past the field, far past it
    flag = n                                                                     # 1 + the last position
    nxt = rng.integers(-5, 1000, size=(B, F)).astype(np.int32)
    y, grp = rng.integers(0, 2, size=B).astype(np.int16), rng.integers(-1, 9, size=B).astype(np.int64)
    acc0 = np.array([1.5, -2.5, 3.25, np.nan], dtype=np.float64)
    acc0.view(np.uint64)[3] = 0x7FF8_0000_DEAD_BEEF                              # a payload: the last two keep their BITS
    d_ids, d_y, d_grp, d_nxt, d_fd = _dev(cuda, ids), _dev(cuda, y), _dev(cuda, grp), _dev(cuda, nxt), _dev(cuda, fd)
    start = n + 1000 if c["big"] else 0
    for fn in ("cdc_stage_batch", "cdc_stage_batch_next"):
        ids_dst, nxt_dst = Guarded(cuda, n, np.int32, I32_FILL, I32_GUARD), Guarded(cuda, n, np.int32, I32_FILL, I32_GUARD)
        y_dst, grp_dst = Guarded(cuda, B, np.int16, -7, -99), Guarded(cuda, B, np.int64, -7, -99)
        alias = Guarded(cuda, 1, np.int32, start, I32_GUARD)
        step, acc = Guarded(cuda, 1, np.int32, 41, I32_GUARD), _dev(cuda, acc0)
        head = (d_ids.data_ptr(), d_y.data_ptr(), d_grp.data_ptr() if c["group"] else None, ids_dst.ptr, y_dst.ptr, grp_dst.ptr, B, F)
        tail = (d_fd.data_ptr() if c["fd"] else None, alias.ptr if c["fd"] else None)
        if fn == "cdc_stage_batch":
            call(lib, fn, *head, *tail)
        else:
            call(lib, fn, *head, d_nxt.data_ptr() if c["nxt"] else None, nxt_dst.ptr, step.ptr if c["step"] else None, acc.data_ptr(),
                 2 if c["step"] else 0, *tail)
        what = f"{fn} ({B}, {F}) {c}"
        assert np.array_equal(ids_dst.read(what + " ids").reshape(B, F), ids)
        assert np.array_equal(y_dst.read(what + " y"), y)
        if c["group"]:
            assert np.array_equal(grp_dst.read(what + " group"), grp)
        else:
            grp_dst.untouched(what + " group_dst without a group")
        assert int(alias.read(what + " alias flag")[0]) == (max(start, flag) if c["fd"] else start)
        got_acc = acc.cpu().numpy()
        if fn == "cdc_stage_batch_next" and c["nxt"]:
            assert np.array_equal(nxt_dst.read(what + " next ids").reshape(B, F), nxt)
        else:
            nxt_dst.untouched(what + " next_dst without next ids")
        if fn == "cdc_stage_batch_next" and c["step"]:
            assert int(step.read(what + " step")[0]) == 42, "the step rises by exactly one"
            assert got_acc[:2].tobytes() == np.zeros(2).tobytes() and got_acc[2:].tobytes() == acc0[2:].tobytes()
        else:
            step.untouched(what + " step")
            assert got_acc.tobytes() == acc0.tobytes()


def test_stage_batch_clean_ids_leave_the_flag(cuda, lib):
    B, F = 300, 7
    rng = np.random.default_rng(3)
    fd = rng.integers(3, 50, size=F).astype(np.int32)
    ids = np.stack([rng.integers(0, d, size=B) for d in fd], axis=1).astype(np.int32)
    ids[:, 0], ids[0, 1] = fd[0] - 1, 0                                          # the last and the first id of a field
    y = np.zeros(B, dtype=np.int16)
    ids_dst, y_dst = Guarded(cuda, B * F, np.int32, I32_FILL, I32_GUARD), Guarded(cuda, B, np.int16, -7, -99)
    alias = Guarded(cuda, 1, np.int32, 0, I32_GUARD)
    d_ids, d_y, d_fd = _dev(cuda, ids), _dev(cuda, y), _dev(cuda, fd)
    call(lib, "cdc_stage_batch", d_ids.data_ptr(), d_y.data_ptr(), None, ids_dst.ptr, y_dst.ptr, None, B, F, d_fd.data_ptr(), alias.ptr)
    assert int(alias.read("alias flag")[0]) == 0 and np.array_equal(ids_dst.read("ids").reshape(B, F), ids)


# ------------------------------------------------------------------------------------------------------------------------
# fills, the in-place addition, the step counter
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1001, 2048 * 256 + 77])
def test_fill_f32_and_f64(cuda, lib, n):
    for name, dtype, value in (("cdc_fill_f32", np.float32, -3.5), ("cdc_fill_f64", np.float64, 1.0 + 2.0 ** -40)):
        buf = Guarded(cuda, n, dtype, np.nan, OUT_SENTINEL)
        call(lib, name, buf.ptr, value, n)
        got = buf.read(name)
        assert got.tobytes() == np.full(n, value, dtype=dtype).tobytes(), f"{name} n={n}"
    t = torch.zeros(4, device=cuda)
    assert lib.cdc_fill_f32(t.data_ptr(), 1.0, -1, _stream()) == BADARG and lib.cdc_fill_f64(None, 1.0, 4, _stream()) == BADARG


@pytest.mark.parametrize("rows,cols", [(0, 5), (7, 63), (4100, 257)])
def test_add_inplace(cuda, lib, rows, cols):
    """(4100, 257): past the 4096 x 256 grid.  One fp32 addition per element; rows = 0 launches nothing."""
    rng = np.random.default_rng(rows + cols)
    a, b = rng.standard_normal((max(rows, 1), cols)).astype(np.float32), rng.standard_normal((max(rows, 1), cols)).astype(np.float32)
    dst, src = PadBuf(cuda, a, out=True), PadBuf(cuda, b, pad=5)
    call(lib, "cdc_add_inplace", dst.ptr, dst.ld, src.ptr, src.ld, rows, cols)
    assert_bits_equal(dst.read("add_inplace dst"), a + b if rows else a, f"add_inplace ({rows}, {cols})")


def test_step_increment(cuda, lib):
    step = Guarded(cuda, 1, np.int32, 41, I32_GUARD)
    call(lib, "cdc_step_increment", step.ptr)
    assert int(step.read("step")[0]) == 42
    call(lib, "cdc_step_increment", step.ptr)
    assert int(step.read("step")[0]) == 43
    assert lib.cdc_step_increment(None, _stream()) == BADARG
