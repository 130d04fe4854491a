"""cdc_gemm_bf16_nt (k_g2_nt, csrc/gemm2.hip), cdc_weight_shadows and cdc_shadow_bf16 straight through the C-ABI against
tests/gemm2_ref.py (float64, derived bounds capped by the suite's present figures), with the conventions of
tests/test_gpu_glinear.py: a sentinel that must survive in output padding (the columns before and behind a row, a row below M),
NaN in the operands' columns at and beyond Kr, plain stores into NaN, accumulate targets pre-filled with random values.

Every case runs under tile_cfg 0 and under every forced class 1..10, in two layouts ("a": every pointer on the 16-byte grid,
ldy % 4 == 0, ldyh % 8 == 0, the mask likewise; "m": ldy = N + 3, an odd ldyh pad and every base one element off the grid) and
with the K padding [K, Kr) both ways round (zeros in A and finite garbage, +-1e30 and +-bf16 max, in B; and the reverse).  All
of these 44 launches are bit-equal to each other: the accumulation order of an element, the dropout keys and the partial sums
depend on neither the tile, the ring depth nor the epilogue path.

Which test reaches which branch, and how it knows:
  * the tile class and ring depth: forced (tile_cfg); what 0 chooses is gemm2_ref.auto_class, held to the launcher's four branches
    by test_automatic_choice (counted tiles asserted on the CPU);
  * the counted vmcnt wait against the vmcnt(0) tail: test_ring (1, 2, 3, 4, 5, 7 slabs under depths 2, 3, 4: totals below the
    depth, and total - t - 1 on both sides of depth - 2); the ring across a segment change: test_segments (seg_32: a change at
    every ring position of every depth, asserted on the CPU);
  * the eight-column forward path against the element-wise one: layout "a" against "m"; inside "a" the pieces that straddle N
    (N = 5, 65, 129) or act_cols = 36 are element-wise; dropout in both (ckey / rkey against g2_drop_bits): test_many_outputs;
  * the bf16-mask prefetch branch: layout "a", mode 1, mask "h", act_cols = width, no accumulate (test_grad_input_epilogues;
    M = 65 and 1 under a 128-row class: passes beyond row_end); the generic vector branch: the same with accumulate, or mask "f",
    or no mask; the element-wise grad-input with a bf16 mask: layout "m", and act_cols = 3 or width - 10 in layout "a";
  * find_group, the lane-held segment list, M = 0 beside live outputs, yh-only / y-only: test_many_outputs, test_forward_geometry;
  * a bias off the 16-byte grid: test_bias_alignment."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm2_ref as R
from bn_ref import bf16_bits, bf16_from_bits, bf16_round
from helpers import OUT_SENTINEL, PadBuf, PadBufH, assert_bits_equal

pytestmark = pytest.mark.gpu
BADARG, ALIGN = -1, -3
CFGS = tuple(range(11))
WS_SENTINEL = -12345.5
_REF = {}


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ref(c):
    """the float64 reference of a launch, computed once and shared"""
    if c["name"] not in _REF:
        D = R.make_data(c)
        _REF[c["name"]] = (D, R.ref(c, D))
    return _REF[c["name"]]


GARBAGE = np.array([1e30, -1e30, 3.3895314e38, -3.3895314e38], dtype=np.float32)     # finite in bf16 (the last two: its largest)


def operand(dev, v, K, zero):
    """[rows, Kr] bf16 in a [rows, Kr + 8] allocation: the columns [K, Kr) zero or finite garbage, those from Kr on NaN"""
    full = np.zeros((v.shape[0], R.r64(K)), np.float32)
    full[:, :K] = v
    if not zero:
        full[:, K:] = GARBAGE[(np.arange(v.shape[0])[:, None] + np.arange(R.r64(K) - K)[None, :]) % 4]
    return PadBufH(dev, full, pad=8)


class Launch:
    """the buffers of one case in one layout with one orientation of the K padding, and its argument block"""

    def __init__(self, dev, c, D, lay, zero="a", bias_shift=0):
        from cdcmdr_amd import _lib as L
        self.c, self.dev, self.lay = c, dev, lay
        self.Lo = R.layout(c, lay)
        self.A = {op: operand(dev, D["a"][op], D["a"][op].shape[1], zero == "a") for op in D["a"]}
        self.B = {op: operand(dev, D["b"][op], D["b"][op].shape[1], zero == "b") for op in D["b"]}
        self.Y, self.YH, self.MASK, self.BIAS = {}, {}, {}, {}
        self.bias_shift = bias_shift
        for o, (O, Lo) in enumerate(zip(c["outs"], self.Lo)):
            M, N, off = O["M"], O["N"], Lo["off"]
            lead = lambda fill: np.full((M, off), fill, np.float32)
            if "y" in O["kind"]:
                v = np.concatenate([lead(OUT_SENTINEL), D["y0"][o] if O["acc"] else np.full((M, N), np.nan, np.float32)], 1)
                v = np.concatenate([v, np.full((1, off + N), OUT_SENTINEL, np.float32)], 0)          # a row below M
                self.Y[o] = PadBuf(dev, v, out=True, pad=Lo["ldy"] - off - N)
            if "h" in O["kind"]:
                v = np.concatenate([lead(OUT_SENTINEL), np.full((M, N), np.nan, np.float32)], 1)
                self.YH[o] = PadBufH(dev, v, out=True, pad=Lo["ldyh"] - off - N, extra_rows=1)
            if O["mask"] is not None:
                v = np.concatenate([lead(np.nan), D["mask"][o]], 1)
                self.MASK[o] = (PadBufH if O["mask"] == "h" else PadBuf)(dev, v, pad=Lo["ldmask"] - off - N)
            if O["bias"]:
                b = np.concatenate([np.full(bias_shift, np.nan, np.float32), D["bias"][o], np.full(1, np.nan, np.float32)])
                self.BIAS[o] = torch.from_numpy(b).to(dev)
        self.ws = None
        if any(O["bn"] is not None for O in c["outs"]):
            self.blocks = max(-(-O["M"] // 64) for O in c["outs"] if O["bn"] is not None)
            self.ws = torch.full((self.blocks + 2, c["bn_total"], 2), WS_SENTINEL, dtype=torch.float64, device=dev)
        self.step = torch.tensor([c["step"] or 0], dtype=torch.int32, device=dev)
        self.a = R.fill_args(L.G2Args(), c, lay, self.ptr)
        self.outputs = list(self.Y.values()) + list(self.YH.values())

    def ptr(self, kind, i):
        if kind == "bias":
            return self.BIAS[i].data_ptr() + 4 * self.bias_shift
        if kind in ("bn", "step"):
            return (self.ws if kind == "bn" else self.step).data_ptr()
        return {"y": self.Y, "yh": self.YH, "mask": self.MASK, "a": self.A, "b": self.B}[kind][i].ptr

    def reset(self):
        for b in self.outputs:
            h = b.host0
            b.t.copy_(torch.from_numpy(h.view(np.int16) if h.dtype == np.uint16 else h))
        if self.ws is not None:
            self.ws.fill_(WS_SENTINEL)

    def call(self, lib, cfg=0):
        self.a.tile_cfg = cfg
        return lib.cdc_gemm_bf16_nt(C.byref(self.a), _stream())

    def untouched(self):
        torch.cuda.synchronize()
        for b in self.outputs:
            h = b.t.cpu().numpy()
            if not np.array_equal(h.view(np.uint16) if b.host0.dtype == np.uint16 else h.view(np.int32),
                                  b.host0 if b.host0.dtype == np.uint16 else b.host0.view(np.int32)):
                return False
        return self.ws is None or bool((self.ws == WS_SENTINEL).all())

    def run(self, lib, cfg=0):
        from cdcmdr_amd import _lib as L
        self.reset()
        L.check(self.call(lib, cfg), "gemm_bf16_nt")
        return self.results()

    def results(self):
        got, c = {}, self.c
        for o, (O, Lo) in enumerate(zip(c["outs"], self.Lo)):
            M, off = O["M"], Lo["off"]
            for key, bufs in (("y", self.Y), ("yh", self.YH)):
                if o not in bufs:
                    continue
                h = bufs[o].read(f"{c['name']} {key}{o}")                    # (checks the columns behind N, and yh's rows below M)
                sent = OUT_SENTINEL if key == "y" else float(bf16_round(np.float32(OUT_SENTINEL)))
                assert (h[:, :off] == sent).all() and (h[M:] == sent).all(), f"{c['name']} {key}{o}: wrote before a row or below M"
                got[f"{key}{o}"] = h[:M, off:]
            if O["bn"] is not None:
                w = self.ws.cpu().numpy()
                blocks = -(-M // 64)
                got[f"bn1_{o}"], got[f"bn2_{o}"] = w[:blocks, O["bn"]:O["bn"] + O["N"], 0].copy(), w[:blocks, O["bn"]:O["bn"] + O["N"], 1].copy()
        if self.ws is not None:
            w = self.ws.cpu().numpy().copy()
            for O in c["outs"]:
                if O["bn"] is not None:
                    w[:-(-O["M"] // 64), O["bn"]:O["bn"] + O["N"]] = WS_SENTINEL
            assert (w == WS_SENTINEL).all(), f"{c['name']}: partial sums outside the outputs' columns and blocks"
        return got


def same_bits(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if a[k].dtype == np.float64:
            assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), f"{what} {k}: bits differ"
        else:
            assert_bits_equal(a[k], b[k], f"{what} {k}")


def run_all(lib, dev, c, lays="am", zeros="ab", cfgs=CFGS):
    """every layout, orientation of the K padding and tile class: within the bounds, and bit-equal to the first"""
    D, W = ref(c)
    first = None
    for lay in lays:
        for zero in zeros:
            la = Launch(dev, c, D, lay, zero)
            for cfg in cfgs:
                got = la.run(lib, cfg)
                what = f"{c['name']}/cfg{cfg}/{lay}/zero-{zero}"
                R.check(c, got, W, what)
                if first is None:
                    first = got
                same_bits(first, got, f"{what} against cfg{cfgs[0]}/{lays[0]}/zero-{zeros[0]}")
    return first


GEO, SEG, GI, MANY, AUTO = R.geometry_cases(), R.segment_cases(), R.gradin_cases(), R.many_cases(), R.auto_cases()
ids = lambda cs: [c["name"] for c in cs]


@pytest.mark.parametrize("c", GEO, ids=ids(GEO))
def test_forward_geometry(cuda, lib, c):
    run_all(lib, cuda, c)


def test_ring(cuda, lib):
    run_all(lib, cuda, R.ring_case())


@pytest.mark.parametrize("c", SEG, ids=ids(SEG))
def test_segments(cuda, lib, c):
    run_all(lib, cuda, c)


@pytest.mark.parametrize("c", GI, ids=ids(GI))
def test_grad_input_epilogues(cuda, lib, c):
    got = run_all(lib, cuda, c)
    D, _ = ref(c)
    for o, O in enumerate(c["outs"]):                          # a masked element without += is 0 exactly, whatever the mask's zero
        if O["mask"] is not None and not O["acc"] and O["act"] > 0:
            off = ~(D["mask"][o][:, :O["act"]] > 0)
            assert not got[("y" if "y" in O["kind"] else "yh") + str(o)][:, :O["act"]][off].any()


@pytest.mark.parametrize("c", MANY, ids=ids(MANY))
def test_many_outputs(cuda, lib, c):
    got = run_all(lib, cuda, c)
    dropped = 0
    for o, O in enumerate(c["outs"]):
        a = min(O["act"], O["N"])
        k = R.keep(c, o)[:, :a]
        v = got[("y" if "y" in O["kind"] else "yh") + str(o)][:, :a]
        assert not v[~k].any(), f"{c['name']} output {o}: a dropped element is not 0"
        if not c["relu"]:                                      # without relu a kept element is 0 only by accident: the exact pattern
            assert (v[k] != 0).all(), f"{c['name']} output {o}: a kept element is 0"
        dropped += int((~k).sum())
    assert dropped > 1000


def test_bn_partials(cuda, lib):
    run_all(lib, cuda, R.bn_case())


@pytest.mark.parametrize("c", AUTO, ids=ids(AUTO))
def test_automatic_choice(cuda, lib, c):
    """what the library chooses by itself (asserted to be class c["expect"] from the counted tiles) equals that class forced, and
    another one"""
    assert R.auto_class(c) == c["expect"]
    other = 10 if c["expect"] != 10 else 9
    run_all(lib, cuda, c, lays="a", zeros="a", cfgs=(0, c["expect"], other))


def test_bias_alignment(cuda, lib):
    """a bias one float off the 16-byte grid in layout "a" (everything else aligned): bit-equal to the aligned run"""
    for c in (GEO[6], R.ring_case()):
        D, W = ref(c)
        want = Launch(cuda, c, D, "a").run(lib, 0)
        for cfg in (0, 1, 7):
            got = Launch(cuda, c, D, "a", bias_shift=1).run(lib, cfg)
            R.check(c, got, W, f"{c['name']}/cfg{cfg}/a/bias+1")
            same_bits(want, got, f"{c['name']}/cfg{cfg} with a bias one float off the 16-byte grid")


# ------------------------------------------------------------------------------------------------------------------------
# argument checks: the documented error code before any launch, every buffer untouched
# ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(cuda, lib):
    fwd = R.case("args_f", 0, [R.out(65, 72, bias=True, act=36, kind="yh"), R.out(3, 8, kind="y", bn=0)], [(100, 0), (64, 1)], bn_total=8)
    gi = R.case("args_x", 1, [R.out(65, 72, act=36, mask="h", kind="yh", acc=1)], [(100, 0)], mask_scale=1.25)

    def refused(c, code, mutate, text=None):
        la = Launch(cuda, c, R.make_data(c), "a")
        mutate(la.a)
        rc = la.call(lib)
        assert rc == code, (c["name"], text, rc, lib.cdc_last_error())
        if text:
            assert text.encode() in (lib.cdc_last_error() or b""), lib.cdc_last_error()
        assert la.untouched(), f"a refused launch wrote ({text})"

    def set_(path, value):
        def f(a):
            obj = a
            for p in path[:-1]:
                obj = getattr(obj, p) if isinstance(p, str) else obj[p]
            setattr(obj, path[-1], value)
        return f

    for n in (0, 25):
        refused(fwd, BADARG, set_(("n_out",), n), "bad counts")
    for n in (0, 33):
        refused(fwd, BADARG, set_(("n_seg",), n), "bad counts")
    refused(fwd, BADARG, set_(("mode",), 2), "mode must be")
    refused(fwd, BADARG, set_(("drop_p",), 1.0), "dropout p out of range")
    for kr in (0, 32):
        refused(fwd, BADARG, set_(("s", 0, "Kr"), kr), "segment 0 malformed")
    refused(fwd, BADARG, set_(("s", 1, "lda"), 56), "segment 1 malformed")
    refused(fwd, BADARG, set_(("s", 1, "out"), 2), "segment 1 malformed")
    refused(fwd, ALIGN, lambda a: setattr(a.s[0], "a", a.s[0].a + 2), "16-byte aligned")
    refused(fwd, ALIGN, lambda a: setattr(a.s[1], "b", a.s[1].b + 2), "16-byte aligned")
    refused(fwd, ALIGN, set_(("s", 0, "lda"), 128 + 4), "16-byte aligned")
    refused(fwd, BADARG, lambda a: (setattr(a.o[0], "y", None), setattr(a.o[0], "yh", None)), "output 0 malformed")
    refused(fwd, BADARG, set_(("o", 0, "ldy"), 71), "output 0 malformed")
    refused(fwd, BADARG, set_(("o", 0, "ldyh"), 71), "output 0 malformed")
    refused(fwd, BADARG, set_(("o", 1, "act_cols"), 1), "cannot feed BatchNorm partial sums")
    refused(fwd, BADARG, set_(("o", 1, "bn_col0"), 1), "cannot feed BatchNorm partial sums")
    refused(gi, BADARG, set_(("o", 0, "y"), None), "accumulates without an fp32 destination")
    ws = torch.full((4, 72, 2), WS_SENTINEL, dtype=torch.float64, device=cuda)
    refused(gi, BADARG, lambda a: (setattr(a.o[0], "bn_partial", ws.data_ptr()), setattr(a.o[0], "bn_total_c", 72), setattr(a.o[0], "act_cols", 0)),
            "cannot feed BatchNorm partial sums")
    assert bool((ws == WS_SENTINEL).all())
    # every M == 0: nothing to do, 0, nothing written
    for c in (fwd, gi):
        la = Launch(cuda, c, R.make_data(c), "a")
        for o in range(la.a.n_out):
            la.a.o[o].M = 0
        assert la.call(lib) == 0 and la.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# cdc_weight_shadows and cdc_shadow_bf16
# ------------------------------------------------------------------------------------------------------------------------
SENT16 = int(bf16_bits(np.array([OUT_SENTINEL], np.float32))[0])
# values exactly between two bf16 numbers (ties to even, both ways), infinities, the largest finite value, denormals
SPECIAL = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000001, 0x00008000, 0x3F807FFF,
                    0x3F808001, 0x80000000], dtype=np.uint32).view(np.float32)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def test_weight_shadows_48_tensors(cuda, lib):
    from cdcmdr_amd import _lib as L
    rng = np.random.default_rng(48)
    shapes = [(1, 1)] + [(r, c) for r in (31, 32, 33) for c in (31, 32, 33)] + [(65, 100), (1, 77), (64, 1), (3, 130), (129, 5), (40, 64)]
    shapes = [shapes[i % len(shapes)] for i in range(46)]
    a = L.WShadowArgs()
    a.n = 48
    keep, checks = [], []

    def dest(rows, cols, pad):
        host = np.full((rows + 1, cols + pad), SENT16, np.uint16)
        return host, torch.from_numpy(host.view(np.int16).copy()).to(cuda)

    def tensor(i, shape):
        w = rng.standard_normal(shape).astype(np.float32)
        k = min(SPECIAL.size, w.size)
        w.ravel()[rng.permutation(w.size)[:k]] = SPECIAL[:k]
        keep.append(torch.from_numpy(w).to(cuda))
        T = a.t[i]
        T.src, T.rows, T.cols = keep[-1].data_ptr(), shape[0], shape[1]
        return w, T

    for i, shape in enumerate(shapes):
        w, T = tensor(i, shape)
        N, K = shape
        if i % 3 != 1:                                          # dst_h only (i % 3 == 0), dst_t only (1), both (2)
            host, dev = dest(N, K, 3 + i % 5)
            T.dst_h, T.ld_h = dev.data_ptr(), host.shape[1]
            host[:N, :K] = bf16_bits(w).reshape(N, K)
            checks.append((f"tensor {i} {shape} dst_h", host, dev))
        if i % 3 != 0:
            host, dev = dest(K, N, 1 + i % 7)
            T.dst_t, T.ld_t = dev.data_ptr(), host.shape[1]
            host[:K, :N] = bf16_bits(w.T).reshape(K, N)
            checks.append((f"tensor {i} {shape} dst_t", host, dev))
    # two tensors [33, 40] and [31, 40] side by side in ONE transposed destination [40, 33 + 31 (+ padding)]
    host, dev = dest(40, 64, 8)
    for i, (n, col) in zip((46, 47), ((33, 0), (31, 33))):
        w, T = tensor(i, (n, 40))
        T.dst_t, T.ld_t = dev.data_ptr() + 2 * col, host.shape[1]
        host[:40, col:col + n] = bf16_bits(w.T).reshape(40, n)
    checks.append(("two tensors in one transposed destination", host, dev))
    L.check(lib.cdc_weight_shadows(C.byref(a), _stream()), "weight_shadows")
    for what, host, dev in checks:
        assert np.array_equal(_u16(dev), host), f"{what}: not the round-to-nearest-even bf16 of the tensor, or its padding written"


def test_shadow_bf16_32_views(cuda, lib):
    from cdcmdr_amd import _lib as L
    rng = np.random.default_rng(32)
    a = L.ShadowArgs()
    a.n = 32
    keep, checks, by_shape = [], [], {}
    combos = [(cols, so, do) for cols in (1, 7, 8, 9, 77) for so in (0, 1) for do in (0, 1)]        # 20 views
    views = [(33 if i % 2 else 301, *cb) for i, cb in enumerate(combos)]
    views.insert(5, (0, 8, 0, 0))                               # rows = 0 between live ones
    views.insert(17, (0, 77, 1, 1))
    views += [(1, cols, so, so) for cols in (1, 8, 9, 77, 16) for so in (0, 1)]
    assert len(views) == 32
    for i, (rows, cols, so, do) in enumerate(views):
        ld_s, ld_d = cols + (-cols) % 4 + 4, cols + (-cols) % 8 + 8     # rows on the 16-byte grid: the offsets alone decide the branch
        x = by_shape.setdefault((rows, cols), rng.standard_normal((rows, cols)).astype(np.float32))
        if x.size >= SPECIAL.size:
            x.ravel()[:SPECIAL.size] = SPECIAL
        src = np.full(so + (rows + 1) * ld_s, np.nan, np.float32)
        src[so:so + rows * ld_s].reshape(rows, ld_s)[:, :cols] = x
        host = np.full(do + (rows + 1) * ld_d, SENT16, np.uint16)
        dev = torch.from_numpy(host.view(np.int16).copy()).to(cuda)
        host[do:do + rows * ld_d].reshape(rows, ld_d)[:, :cols] = bf16_bits(x).reshape(rows, cols)
        keep.append(torch.from_numpy(src).to(cuda))
        T = a.t[i]
        T.src, T.ld_src, T.dst, T.ld_dst, T.rows, T.cols = keep[-1].data_ptr() + 4 * so, ld_s, dev.data_ptr() + 2 * do, ld_d, rows, cols
        checks.append((f"view {i} rows {rows} cols {cols} src+{so} dst+{do}", host, dev))
    L.check(lib.cdc_shadow_bf16(C.byref(a), _stream()), "shadow_bf16")
    for what, host, dev in checks:                              # the same expected bits for the vector and the scalar branch
        assert np.array_equal(_u16(dev), host), f"{what}: not the round-to-nearest-even bf16 of the view, or its padding written"
