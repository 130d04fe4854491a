"""cdc_glinear_bwd_xw (csrc/gemm2.hip k_g2_xw): a grad-input launch and the two grad-weight classes behind it as ONE launch,
against the two calls it replaces — cdc_gemm_bf16_nt, then cdc_glinear_bwd_w_pair — bit for bit.

Every workgroup of the fused launch runs the body of the launch it comes from on the same operands in the same order, so
nothing may differ: both forms write into buffers pre-filled identically (a NaN pattern where nothing accumulates, equal random
values where something does, and in what a deferred launch must leave alone) and every output is compared on its raw bytes,
guards and padding included: dX in fp32, its bf16 shadow, every float of both slab regions, dw / db.

Shapes, the smallest that reach every branch.  M = 200: a ragged last 64-row slab, shadows zero-padded to 256 rows; wide
groups (N, K) = (256, 416) and (128, 256) with split_k 3, deferred; narrow groups (64, 128) and (3, 416) with split_k 2
deferred, or split_k 1 (dw / db written, one group accumulates); grad-input with 64 x 64 tiles (tile_cfg 9, what the flagship's
launch takes): one output [200 x 416] from three segments Kr = 256, 256, 64, without and with accumulate, or two outputs — N =
256 behind a bf16 ReLU mask, N = 128 in fp32 and as a shadow.  The three block counts are 30, 18 (9 unsplit) and 28: none a
multiple of 8 (the XCD remap of each body's LOCAL index), one below 32.  M = 64: one slab, split_k 1 everywhere.
The 128 x 128 grad-input class (tile_cfg 1) runs the M = 200 case once.

Refusals (return code, nothing written): a null block, a narrow group with N > 64, a grad-input output aliased onto a dzh, and
a grad-input tile class the fused kernel is not instantiated for."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN32 = 0x7FC0BEEF                          # quiet NaNs with payloads no kernel produces
NAN16 = 0x7FC5
GUARD = 64                                  # elements on each side of every output
BADARG = -1                                 # CDC_E_BADARG


def r64(n):
    return (n + 63) // 64 * 64


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """an output of `n` elements (fp32, or bf16 when half) between two guard regions: NaN pattern, or `values`"""

    def __init__(self, dev, n, half=False, values=None):
        dt, pat = (np.uint16, NAN16) if half else (np.uint32, NAN32)
        h = np.full(n + 2 * GUARD, pat, dtype=dt)
        if values is not None:
            h[GUARD:GUARD + n] = np.ascontiguousarray(values, dtype=np.float32).ravel().view(np.uint32)
        self.t = torch.from_numpy(h.view(np.int16 if half else np.int32)).to(dev)
        self.ptr = self.t.data_ptr() + GUARD * (2 if half else 4)
        self.n, self.pat = n, pat

    def live(self):
        return self.t[GUARD:GUARD + self.n]


def shadow(dev, rng, rows, cols, pad_nan=True):
    """bf16 operand as plan.py allocates shadows: rows to a multiple of 64 (zero past `rows`), columns to a multiple of 64 plus 64
    (NaN in the live rows' padding: nothing may leak from it)"""
    s = torch.zeros((r64(rows), r64(cols) + 64), dtype=torch.bfloat16, device=dev)
    if pad_nan:
        s[:rows, cols:] = float("nan")
    s[:rows, :cols] = torch.from_numpy(rng.standard_normal((rows, cols)).astype(np.float32)).to(dev).to(torch.bfloat16)
    return s


class Inputs:
    """the read-only operands of a case, shared by the two forms"""

    def __init__(self, dev, M, wide, narrow, outs):
        rng = np.random.default_rng(1234 + M)
        self.M, self.wide, self.narrow, self.outs = M, wide, narrow, outs
        self.dw = {(c, g): (shadow(dev, rng, M, N), shadow(dev, rng, M, K)) for c, gs in (("w", wide), ("n", narrow))
                   for g, (N, K, _db) in enumerate(gs)}
        # grad-input: A [M, Kr] (whole K slabs: no padding inside Kr), B [N, Kr] (the W^T copies), a bf16 mask per masked output
        self.seg = [[(shadow(dev, rng, M, Kr, pad_nan=False), shadow(dev, rng, N, Kr, pad_nan=False)) for Kr in krs] for N, krs, *_ in outs]
        self.mask = [shadow(dev, rng, M, N) if masked else None for N, _k, masked, *_ in outs]
        self.start = {}                     # equal random starting values of whatever accumulates or must be left alone

    def values(self, key, n):
        if key not in self.start:
            self.start[key] = np.random.default_rng(zlib.crc32(repr(key).encode())).standard_normal(n).astype(np.float32)
        return self.start[key]


class Form:
    """argument blocks and output buffers of one form (two launches, or the fused one) of a case"""

    def __init__(self, dev, I, split_w, split_n, accumulate, tile_cfg):
        from cdcmdr_amd import _lib as L
        self.I, self.bufs = I, {}
        M = I.M
        x = self.x = L.G2Args()
        x.n_out, x.mode, x.relu, x.drop_p, x.mask_scale, x.tile_cfg = len(I.outs), 1, 0, 0.0, 1.25, tile_cfg
        si = 0
        for o, (N, krs, masked, want_y, want_h) in enumerate(I.outs):
            O = x.o[o]
            O.M, O.N, O.accumulate, O.stream_id = M, N, accumulate if want_y else 0, o
            if want_y:
                b = self.bufs[f"dx{o}"] = Out(dev, M * (N + 4), values=I.values(("dx", o), M * (N + 4)) if accumulate else None)
                O.y, O.ldy = b.ptr, N + 4
            if want_h:
                b = self.bufs[f"dxh{o}"] = Out(dev, M * (N + 8), half=True)
                O.yh, O.ldyh = b.ptr, N + 8
            if masked:
                O.mask, O.ldmask, O.mask_bf16, O.act_cols = I.mask[o].data_ptr(), I.mask[o].stride(0), 1, N
            for (A, B), Kr in zip(I.seg[o], krs):
                S = x.s[si]
                S.a, S.lda, S.b, S.ldb, S.Kr, S.out = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), Kr, o
                si += 1
        x.n_seg = si
        self.blocks = []
        for c, groups, split in (("w", I.wide, split_w), ("n", I.narrow, split_n)):
            a = L.LinBwdwArgs()
            a.n_groups, a.split_k, a.defer_reduce = len(groups), split, 1 if split > 1 else 0
            slab = sum(N * K + N for N, K, _db in groups)
            if split > 1:
                b = self.bufs[f"slabs_{c}"] = Out(dev, split * slab)
                a.workspace = b.ptr
            for g, (N, K, has_db) in enumerate(groups):
                G = a.g[g]
                acc = 1 if (split == 1 and g == 1) else 0
                start = acc or split > 1                              # accumulated into, or left alone by a deferred launch
                b = self.bufs[f"dw_{c}{g}"] = Out(dev, N * K, values=I.values(("dw", c, g), N * K) if start else None)
                G.dw, G.lddw, G.M, G.N, G.K, G.accumulate = b.ptr, K, M, N, K, acc
                if has_db:
                    b = self.bufs[f"db_{c}{g}"] = Out(dev, N, values=I.values(("db", c, g), N) if start else None)
                    G.db = b.ptr
                dzh, xh = I.dw[c, g]
                G.dzh, G.lddzh, G.xh, G.ldxh = dzh.data_ptr(), dzh.stride(0), xh.data_ptr(), xh.stride(0)
            self.blocks.append(a)
        self.tabs = torch.frombuffer(bytearray(bytes(self.blocks[0]) + bytes(self.blocks[1])), dtype=torch.uint8).to(dev)

    def two_launches(self, lib):
        from cdcmdr_amd import _lib as L
        L.check(lib.cdc_gemm_bf16_nt(C.byref(self.x), stream()), "cdc_gemm_bf16_nt")
        L.check(lib.cdc_glinear_bwd_w_pair(C.byref(self.blocks[0]), C.byref(self.blocks[1]), C.c_void_p(self.tabs.data_ptr()), stream()),
                "cdc_glinear_bwd_w_pair")

    def fused(self, lib):
        return lib.cdc_glinear_bwd_xw(C.byref(self.x), C.byref(self.blocks[0]), C.byref(self.blocks[1]), C.c_void_p(self.tabs.data_ptr()), stream())

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: b.t.clone() for k, b in self.bufs.items()}


WIDE = [(256, 416, 1), (128, 256, 1)]                                  # (N, K, db)
NARROW = [(64, 128, 1), (3, 416, 1)]
ONE_OUT = [(416, (256, 256, 64), False, True, False)]                  # (N, Kr of its segments, bf16 ReLU mask, fp32, shadow)
TWO_OUTS = [(256, (256, 64), True, True, False), (128, (128, 256), False, True, True)]
CASES = {
    "M200-narrow-split2": (200, 3, 2, ONE_OUT, 0, 9),
    "M200-narrow-unsplit-accumulate": (200, 3, 1, ONE_OUT, 1, 9),
    "M200-two-outputs": (200, 3, 2, TWO_OUTS, 0, 9),
    "M200-tiles128": (200, 3, 2, ONE_OUT, 0, 1),
    "M64-one-slab": (64, 1, 1, ONE_OUT, 0, 9),
}
_INPUTS = {}


def inputs(dev, M, outs):
    key = (M, id(outs))
    if key not in _INPUTS:
        _INPUTS[key] = Inputs(dev, M, WIDE, NARROW, outs)
    return _INPUTS[key]


@pytest.mark.parametrize("name", list(CASES))
def test_fused_launch_equals_the_two_launches_bit_for_bit(cuda, lib, name):
    from cdcmdr_amd import _lib as L
    M, split_w, split_n, outs, accumulate, tile_cfg = CASES[name]
    I = inputs(cuda, M, outs)
    two, one = Form(cuda, I, split_w, split_n, accumulate, tile_cfg), Form(cuda, I, split_w, split_n, accumulate, tile_cfg)
    before = one.snapshot()
    assert all(torch.equal(before[k], v) for k, v in two.snapshot().items()), "the two forms do not start from the same bytes"
    two.two_launches(lib)
    L.check(one.fused(lib), "cdc_glinear_bwd_xw")
    want, got = two.snapshot(), one.snapshot()
    assert want.keys() == got.keys()
    for k in want:
        assert torch.equal(want[k], got[k]), f"{name}: {k} differs from the two launches"
    # ... and the launches did write: no output element still holds the pattern (a deferred launch's dw / db hold their values)
    for k, b in one.bufs.items():
        if k.startswith("dx") and not k.startswith("dxh"):
            N = outs[int(k[2:])][0]
            live = b.live().view(M, N + 4)
            assert not (live[:, :N] == NAN32).any(), f"{name}: {k} not written everywhere"
            assert torch.equal(live[:, N:], before[k][GUARD:GUARD + b.n].view(M, N + 4)[:, N:]), f"{name}: {k} padding written"
        if k.startswith("slabs"):
            assert not torch.equal(got[k], before[k]), f"{name}: {k} not written"
        if k.startswith("dw_n") and split_n == 1:
            assert not torch.equal(got[k], before[k]), f"{name}: {k} not written"


def refused(lib, form, rc_want, *args):
    before = form.snapshot()
    rc = lib.cdc_glinear_bwd_xw(*args, stream()) if args else form.fused(lib)
    assert rc == rc_want, f"return code {rc}, expected {rc_want}: {lib.cdc_last_error()}"
    after = form.snapshot()
    assert all(torch.equal(before[k], after[k]) for k in before), "a refused launch wrote something"


def test_refusals(cuda, lib):
    from cdcmdr_amd import _lib as L
    I = inputs(cuda, 200, ONE_OUT)
    f = Form(cuda, I, 3, 2, 0, 9)
    x, w, n, t = C.byref(f.x), C.byref(f.blocks[0]), C.byref(f.blocks[1]), C.c_void_p(f.tabs.data_ptr())
    for args in ((None, w, n, t), (x, None, n, t), (x, w, None, t), (x, w, n, None)):
        refused(lib, f, BADARG, *args)
    # a narrow group with more than 64 output rows
    g = Form(cuda, Inputs(cuda, 200, WIDE, [(64, 128, 1), (72, 64, 1)], ONE_OUT), 3, 2, 0, 9)
    refused(lib, g, BADARG)
    # the grad-input output aliased onto a dZ shadow the grad-weight tiles read
    h = Form(cuda, I, 3, 2, 0, 9)
    dzh = I.dw["w", 0][0]
    h.x.o[0].y, h.x.o[0].ldy = dzh.data_ptr(), 416
    keep = dzh.clone()
    refused(lib, h, BADARG)
    assert torch.equal(dzh.view(torch.int16), keep.view(torch.int16))
    # ... and its shadow onto the slab workspace they write
    h2 = Form(cuda, I, 3, 2, 0, 9)
    h2.x.o[0].yh, h2.x.o[0].ldyh = h2.blocks[0].workspace, 416
    refused(lib, h2, BADARG)
    # a tile class the fused kernel has no grad-input body for (the library's own choice for this shape: 64 x 128 tiles)
    k = Form(cuda, I, 3, 2, 0, 0)
    refused(lib, k, BADARG)
    L.check(lib.cdc_gemm_bf16_nt(C.byref(k.x), stream()), "cdc_gemm_bf16_nt")       # (alone it is a valid launch)
    torch.cuda.synchronize()
