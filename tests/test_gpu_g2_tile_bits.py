"""cdc_gemm_bf16_nt (csrc/gemm2.hip): the tile class and ring depth move no bit of any output.

Per output element the K order (segments in launch order, 64-wide slabs, two MFMAs of 32 per slab) and the MFMA instruction are the
same in all ten instantiations, and the epilogue is element-wise — so every forced class (cdc_g2_args.tile_cfg 1..10), and whatever
the launcher chooses by itself (tile_cfg 0), must give the fp32 and bf16 outputs of class 9 bit for bit, whole buffers (the
sentinels behind the N columns included).  That is what lets the launcher's choice follow a measurement alone.  Class 9's own
result is held to the restated arithmetic in double first, so that ten equal wrong answers do not pass.

Shapes: outputs of M = 130 and M = 1 rows (three, two, one row tiles; a tile of one row) with N = 72 and N = 136 columns (the last
column tile ragged for 64 and for 128), three segments of Kr = 64 / 128 / 64 — two of them reducing into one output — whose true
lengths 40 / 100 / 64 leave zero padding in the slabs; one fp32 destination with an odd row stride (element-wise epilogue), one on
the 16-byte grid (vector epilogue).

Class 9 against double, 2e-5 (relative + absolute, tests/test_gpu_gemm2.py's bound): the operands are the same bf16 values on both
sides, so what differs is the fp32 accumulation — at most K / 32 = 18 MFMA steps, each rounding a partial sum below 16 in
magnitude to half an ulp, 18 x 2^-24 x 16 / 2 = 0.9e-5 — and one rounding each of the scale, the bias and the += in the epilogue."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

CFGS = tuple(range(1, 11))
MS, NS = (130, 1), (72, 136)
SEGS = ((40, 0), (100, 0), (64, 1))                                   # (true reduction length, output): Kr = 64, 128, 64
SEED = 0x5EED_0123_4567_89AB


def _r64(n):
    return (n + 63) // 64 * 64


def _shadow(t):
    """zero-padded bf16 copy [rows, cols64 + 64] of an fp32 matrix (rows past M are never read: the kernel clamps them)"""
    rows, cols = t.shape
    s = torch.zeros((rows, _r64(cols) + 64), dtype=torch.bfloat16, device=t.device)
    s[:rows, :cols] = t.to(torch.bfloat16)
    return s


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


class Case:
    """the buffers and the argument block of one launch; run(cfg) -> the raw bits of every output buffer"""

    def __init__(self, dev, mode, Ms, Ns, segs, ldy_extra, accumulate=(), mask_on=(), seed=7):
        from cdcmdr_amd import _lib as L
        gen = torch.Generator().manual_seed(seed)
        self.mode, self.Ms, self.Ns, self.segs = mode, Ms, Ns, segs
        self.A = [_shadow(torch.randn(Ms[o], k, generator=gen).to(dev)) for k, o in segs]
        self.B = [_shadow((torch.randn(Ns[o], k, generator=gen) / k ** 0.5).to(dev)) for k, o in segs]
        self.bias = [torch.randn(n, generator=gen).to(dev) for n in Ns]
        self.mask = [_shadow(torch.randn(m, n, generator=gen).to(dev)) for m, n in zip(Ms, Ns)]      # bf16: the producing layer's activation
        self.old = [torch.randn(m, n + e, generator=gen).to(dev) for m, n, e in zip(Ms, Ns, ldy_extra)]
        self.y = [torch.empty_like(t) for t in self.old]
        self.yh = [torch.empty((m, _r64(n)), dtype=torch.bfloat16, device=dev) for m, n in zip(Ms, Ns)]
        self.accumulate, self.mask_on = accumulate, mask_on
        a = self.a = L.G2Args()
        a.n_out, a.n_seg, a.mode = len(Ms), len(segs), mode
        if mode == 0:
            a.relu, a.drop_p, a.mask_scale, a.seed, a.seed_offset_dev = 1, 0.2, 1.0, SEED, None
        else:
            a.relu, a.drop_p, a.mask_scale, a.seed, a.seed_offset_dev = 0, 0.0, 1.25, 0, None
        for o, (m, n) in enumerate(zip(Ms, Ns)):
            O = a.o[o]
            O.y, O.ldy, O.yh, O.ldyh = self.y[o].data_ptr(), self.y[o].stride(0), self.yh[o].data_ptr(), self.yh[o].stride(0)
            O.M, O.N, O.stream_id = m, n, o
            if mode == 0:
                O.bias, O.act_cols = self.bias[o].data_ptr(), n - 6          # the last 6 columns: bias only
            else:
                O.accumulate = 1 if o in accumulate else 0
                if o in mask_on:
                    O.mask, O.ldmask, O.mask_bf16, O.act_cols = self.mask[o].data_ptr(), self.mask[o].stride(0), 1, n - 10
        for i, (k, o) in enumerate(segs):
            S = a.s[i]
            S.a, S.lda, S.b, S.ldb, S.Kr, S.out = self.A[i].data_ptr(), self.A[i].stride(0), self.B[i].data_ptr(), self.B[i].stride(0), _r64(k), o

    def run(self, lib, cfg):
        from cdcmdr_amd import _lib as L
        for o in range(len(self.Ms)):
            if o in self.accumulate:
                self.y[o].copy_(self.old[o])
            else:
                self.y[o].fill_(float("nan"))
            self.yh[o].fill_(float("nan"))
        self.a.tile_cfg = cfg
        L.check(lib.cdc_gemm_bf16_nt(C.byref(self.a), _stream()), "gemm_bf16_nt")
        torch.cuda.synchronize()
        return [_bits(t) for t in self.y + self.yh]

    def products(self):
        """the contractions in double on the bf16 operands, per output"""
        want = [torch.zeros(m, n, dtype=torch.float64) for m, n in zip(self.Ms, self.Ns)]
        for i, (k, o) in enumerate(self.segs):
            want[o] += self.A[i][:, :k].double().cpu() @ self.B[i][:, :k].double().cpu().t()
        return want


def _all_classes_equal_class_9(lib, case, check_9):
    base = case.run(lib, 9)
    check_9(case)
    for cfg in CFGS:
        got = case.run(lib, cfg)
        for i, (b, g) in enumerate(zip(base, got)):
            kind = "fp32" if i < len(case.Ms) else "bf16"
            assert torch.equal(b, g), f"tile_cfg {cfg}: {kind} output {i % len(case.Ms)} differs from tile_cfg 9 in {int((b != g).sum())} words"


def test_grad_input_bits_do_not_depend_on_the_tile_class(cuda):
    from cdcmdr_amd import _lib as L
    lib = L.load()
    case = Case(cuda, 1, MS, NS, SEGS, ldy_extra=(3, 8), accumulate=(1,), mask_on=(0,))

    def check_9(c):
        want = c.products()
        n0 = NS[0] - 10
        want[0][:, :n0] = want[0][:, :n0] * 1.25 * (c.mask[0][:, :n0] > 0).double().cpu()
        want[1] = want[1] + c.old[1][:, :NS[1]].double().cpu()
        for o in range(2):
            assert_close(c.y[o][:, :NS[o]], want[o], 2e-5, 2e-5, f"dx{o}")
            assert bool(torch.isnan(c.y[0][:, NS[0]:]).all()) and torch.equal(c.y[1][:, NS[1]:], c.old[1][:, NS[1]:]), "wrote past the N columns"
            assert torch.equal(c.yh[o][:, :NS[o]].cpu(), c.y[o][:, :NS[o]].to(torch.bfloat16).cpu()), "the bf16 output is not the rounding of the fp32 one"

    _all_classes_equal_class_9(lib, case, check_9)


def test_forward_bits_do_not_depend_on_the_tile_class(cuda):
    """bias, ReLU and dropout p = 0.2 under a fixed seed: the keep decisions are keyed by (seed, stream, row, column), never by the tile"""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    case = Case(cuda, 0, MS, NS, SEGS, ldy_extra=(3, 8))

    def check_9(c):
        want = c.products()
        kept = pos = 0
        for o in range(2):
            n, act = NS[o], NS[o] - 6
            w = want[o] + c.bias[o].double().cpu()
            y = c.y[o][:, :n].double().cpu()
            assert_close(c.y[o][:, act:n], w[:, act:], 2e-5, 2e-5, f"y{o}, columns without activation")
            on = y[:, :act] != 0                                   # a kept element is relu(x) / (1 - p); a dropped one 0
            assert_close(torch.where(on, y[:, :act], torch.zeros(())), torch.where(on, torch.relu(w[:, :act]) * 1.25, torch.zeros(())), 3e-5, 3e-5, f"y{o}")
            kept += int((on & (w[:, :act] > 1e-3)).sum())
            pos += int((w[:, :act] > 1e-3).sum())
            assert torch.equal(c.yh[o][:, :n].cpu(), c.y[o][:, :n].to(torch.bfloat16).cpu())
        # about 4 700 positive elements: the kept share is 0.8 with a standard deviation of 0.006
        assert pos > 4000 and 0.75 < kept / pos < 0.85, f"{kept} of {pos} positive elements kept under p = 0.2"

    _all_classes_equal_class_9(lib, case, check_9)


def test_the_launchers_own_choice_at_an_under_filled_shape_equals_class_9(cuda):
    """tile_cfg 0 at dX[4096 x 416] over K = 2 x 256 + 64: 128 tiles of 128 x 128 for 256 CUs, the branch of the launcher that
    picks among the 64-row classes"""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    case = Case(cuda, 1, (4096,), (416,), ((256, 0), (256, 0), (64, 0)), ldy_extra=(0,), mask_on=(0,), seed=11)
    base = case.run(lib, 9)
    want = case.products()[0]
    want[:, :406] = want[:, :406] * 1.25 * (case.mask[0][:, :406] > 0).double().cpu()
    assert_close(case.y[0], want, 2e-5, 2e-5, "dx")
    got = case.run(lib, 0)
    for b, g, kind in zip(base, got, ("fp32", "bf16")):
        assert torch.equal(b, g), f"tile_cfg 0: {kind} output differs from tile_cfg 9 in {int((b != g).sum())} words"
