"""The grouped linear launches of csrc/gemm.hip and the shadow grad-weight kernels of csrc/gemm2.hip straight through the C-ABI
against tests/glinear_ref.py (float64, derived bounds capped by the suite's present figures), with the conventions of
tests/test_gpu_head.py: NaN in input padding, a sentinel that must survive in output padding, plain stores into NaN, accumulate
targets pre-filled with random values.  Every case runs in two layouts: "a" (rows padded up to a multiple of 4 floats: the lean
16-byte staging and the float4 epilogues) and "m" (helpers.PAD = 3 extra columns: the generic Stage loads and the scalar
epilogues wherever cols % 4 != 1).  How a case knows its path: the layout (lean / generic), the operand form (w / wt / bf16 wt),
the reduction length (8 tail only, 32 one slab, 40 slab + tail, 64 two slabs in flight, 96 an odd count, 100 the fall-back to
one slab in flight), split_k and the slices glinear_ref.slices restates, the counted tiles (>= 16384: 128 x 128), the shadows.

Bit equalities the code implies are asserted: layout "a" against "m", wt against w, bf16 wt against fp32 wt, the 128 x 128
class against the 64 x 64 class, the pair launches against two single ones, the reduce launch against the host's fp32 sum of the
slabs in slice order.

The 16-byte branch of bwd_w_reduce_body needs a slab stride that is a multiple of 4, and the stride IS the sum of the group
sizes: with every N K and every flat start a multiple of 4, a last group whose N is not a multiple of 4 makes the stride odd and
the launch takes the scalar branch.  The piece of the 16-byte branch for a group that ends mid-quad therefore cannot be reached
through the launchers; the case the issue describes is run all the same (test_reduce_launch, "lastN3").

Which test reaches which path, and how it knows:
  * 128 x 128 tiles, the un-staged epilogue: test_forward_128_class, test_grad_input_128_class (32 ragged groups, M = 65536: the
    test asserts >= 16384 counted tiles), test_forward_128_class_dense_production_shape (512 x 32 tiles);
  * generic Stage loads: layout "m" of every forward / grad-input case (K and N multiples of 4, so K + 3 is not), wt with N = 3, 65;
    LeanStage row clamping and load_tail: layout "a" with 1, 63, 65, 130 rows and reduction lengths 8, 40, 100;
  * the two-slab pipeline: bf16 grad-input in the "wt" / "wth" forms, 64 x 64 class, N = 64 (even), 96 (odd), 100 (falls back);
  * gemm_accumulate_half_b: the "wth" form (bf16 copies written by cdc_transpose_multi), eligibility in
    test_grad_input_argument_checks;
  * the lane-fetched segment list: x_seg32 (32 segments into 3 outputs, interleaved), x_three, x_ragged, x_unnamed;
  * empty and partial split_k slices: test_grad_weight at M = 65 in 8 slices, 31 in 2, 200 in 5, 1000 in 8, per form, each slab
    compared with the slice glinear_ref.slices cuts (32 rows for the fp32 kernel, 64 for the other two);
  * the slab layout under defer_reduce: the *_defer cases of test_grad_weight and the pair tests (check_deferred);
  * both branches of bwd_w_reduce_body and k_bwd_w_reduce_dual: test_reduce_launch, test_pair_reduce_equals_two_split_launches;
  * the three bias gradients: db against the unrounded dz (forms "f32", "tr") or the bf16 dz ("sh"); the CPU test shows the bound
    telling them apart (defect db_kind);
  * ragged groups with an empty one: f_ragged, f_raggeddrop, x_ragged, w_f32_ragged*, w_tr_ragged*;
  * cdc_transpose_multi: test_transpose_multi, and every "wt" / "wth" launch reads its output."""
import ctypes as C

import numpy as np
import pytest
import torch

import glinear_ref as R
from bn_ref import bf16_bits, bf16_round
from helpers import OUT_SENTINEL, PAD, PadBuf, assert_bits_equal, assert_bounded, nan_like

pytestmark = pytest.mark.gpu
PRECS = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F32, id="f32")]
FWD, BWDX = R.fwd_cases(), R.bwdx_cases()
_REF = {}


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    from cdcmdr_amd import _lib as L
    L.check(getattr(lib, name)(*args, _stream()), name)


def ref(tag, c, prec, **kw):
    """the float64 reference of a launch, computed once and shared"""
    key = (tag, c["name"], prec, c.get("defer"), tuple(sorted(kw.items())))
    if key not in _REF:
        D = R.make_data(c)
        _REF[key] = (D, R.ref(tag, c, D, prec, **kw))
    return _REF[key]


def buf(dev, values, lay, out=False, extra=0):
    cols = np.asarray(values).shape[-1]
    return PadBuf(dev, values, out=out, pad=extra + ((-(cols + extra)) % 4 if lay == "a" else PAD))


def i32(dev, v):
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device=dev)


def compare(got, want, what):
    for k, (w, b) in want.items():
        assert k in got, f"{what}: {k} not produced"
        assert_bounded(got[k], w, b, f"{what} {k}")


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert_bits_equal(a[k], b[k], f"{what} {k}")


def _rows_of(full, init, lo, n, what):
    """the group's rows; every other row of the buffer must hold what it held before the launch"""
    rest = np.concatenate([np.arange(0, lo), np.arange(lo + n, full.shape[0])]).astype(np.int64)
    assert np.array_equal(full[rest].view(np.int32), init[rest].view(np.int32)), f"{what}: rows outside the group written"
    return full[lo:lo + n]


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def run_fwd(lib, dev, c, D, prec, lay, M_arg=None):
    from cdcmdr_amd import _lib as L
    a, keep = L.LinFwdArgs(), []
    a.n_groups, a.relu, a.drop_p, a.seed = len(c["Ns"]), c["relu"], c["p"], R.SEED
    if c["step"] is not None:
        keep.append(i32(dev, [c["step"]]))
        a.seed_offset_dev = keep[-1].data_ptr()
    if c["rows"] is not None:
        keep.append(i32(dev, R.offsets(c["rows"])))
        a.row_offsets = keep[-1].data_ptr()
    X, Y = buf(dev, D["x"], lay), []
    for g, N in enumerate(c["Ns"]):
        W, Y_ = buf(dev, D["w"][g], lay), buf(dev, nan_like(c["R"], N), lay, out=True)
        G = a.g[g]
        G.x, G.ldx, G.w, G.ldw, G.y, G.ldy = X.ptr, X.ld, W.ptr, W.ld, Y_.ptr, Y_.ld
        if c["bias"][g]:
            keep.append(buf(dev, D["b"][g], lay))
            G.bias = keep[-1].ptr
        G.M = (M_arg or c["M_arg"] or c["R"]) if c["rows"] is not None else c["Ms"][g]
        G.N, G.K, G.act_cols = N, c["K"], c["act"][g]
        keep.append(W), Y.append(Y_)
    call(lib, "cdc_glinear_fwd", C.byref(a), prec)
    out = {}
    for g in range(len(c["Ns"])):
        lo, n = R.group_rows(c, g)
        out[f"y{g}"] = _rows_of(Y[g].read(f"y{g}"), Y[g].host0[:, :Y[g].cols], lo, n, f"{c['name']} y{g}")
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_forward(cuda, lib, c, prec):
    D, want = ref("fwd", c, prec)
    got = {lay: run_fwd(lib, cuda, c, D, prec, lay) for lay in "am"}
    for lay in "am":
        compare(got[lay], want, f"{c['name']}/{lay}")
    same_bits(got["a"], got["m"], c["name"])
    if c["p"] > 0:                                             # dropped elements are exactly 0, and there are some
        for g in range(len(c["Ns"])):
            lo, n = R.group_rows(c, g)
            drop = ~R.fwd_keep(c, g, lo, n)[:, :c["act"][g]]
            assert not got["a"][f"y{g}"][:, :c["act"][g]][drop].any()
        assert sum(int((~R.fwd_keep(c, g, *R.group_rows(c, g))).sum()) for g in range(len(c["Ns"]))) > 100


# ------------------------------------------------------------------------------------------------------------------------
# grad-input
# ------------------------------------------------------------------------------------------------------------------------
def transposed(lib, dev, mats, half):
    """W^T copies [cols, rows] of dense fp32 matrices through cdc_transpose_multi (bf16 when `half`)"""
    from cdcmdr_amd import _lib as L
    ta, src, dst = L.TransposeArgs(), [], []
    ta.n = len(mats)
    for i, m in enumerate(mats):
        src.append(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dev))
        dst.append(torch.zeros(m.size, dtype=torch.bfloat16, device=dev) if half else torch.full((m.size,), float("nan"), device=dev))
        ta.t[i].src, ta.t[i].dst, ta.t[i].rows, ta.t[i].cols = src[i].data_ptr(), dst[i].data_ptr(), m.shape[0], m.shape[1]
        if half:
            ta.bf16_mask |= 1 << i
    call(lib, "cdc_transpose_multi", C.byref(ta))
    return dst


def run_bwdx(lib, dev, c, D, prec, lay, form, M_arg=None):
    from cdcmdr_amd import _lib as L
    a, keep, DX = L.LinBwdxArgs(), [], []
    a.n_out, a.n_seg, a.mask_scale = len(c["outs"]), len(c["segs"]), c["mask_scale"]
    if c["rows"] is not None:
        keep.append(i32(dev, R.offsets(c["rows"])))
        a.row_offsets = keep[-1].data_ptr()
    for o, (K, mcols, acc) in enumerate(c["outs"]):
        DX.append(buf(dev, D["dx0"][o] if acc else nan_like(c["R"], K), lay, out=True))
        O = a.o[o]
        O.dx, O.lddx, O.K, O.accumulate = DX[o].ptr, DX[o].ld, K, acc
        O.M = (M_arg or c["M_arg"] or c["R"]) if c["rows"] is not None else c["M"]
        if mcols is not None:
            keep.append(buf(dev, D["mask"][o], lay))
            O.mask_y, O.ldmask, O.mask_cols = keep[-1].ptr, keep[-1].ld, mcols
    with_wt = [s for s in range(len(c["segs"])) if form in ("wt", "wth") or (form == "mix" and s % 2 == 0)] if form != "w" else []
    wts = dict(zip(with_wt, transposed(lib, dev, [D["w"][s] for s in with_wt], form == "wth"))) if with_wt else {}
    for s, (N, o) in enumerate(c["segs"]):
        DZ, W = buf(dev, D["dz"][s], lay), buf(dev, D["w"][s], lay)
        S = a.s[s]
        S.dz, S.lddz, S.w, S.ldw, S.N, S.out = DZ.ptr, DZ.ld, W.ptr, W.ld, N, o
        if s in wts:
            S.wt, S.ldwt, S.wt_bf16 = wts[s].data_ptr(), N, int(form == "wth")
        keep += [DZ, W]
    call(lib, "cdc_glinear_bwd_x", C.byref(a), prec)
    out = {}
    for o in range(len(c["outs"])):
        lo, n = R.group_rows(c, o)
        out[f"dx{o}"] = _rows_of(DX[o].read(f"dx{o}"), DX[o].host0[:, :DX[o].cols], lo, n, f"{c['name']} dx{o}")
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c,forms", BWDX, ids=[c["name"] for c, _ in BWDX])
def test_grad_input(cuda, lib, c, forms, prec):
    D, want = ref("bwdx", c, prec)
    got = {}
    for form in forms:
        if form == "wth" and prec != R.BF16:
            continue
        for lay in ("a",) if form == "wth" else "am":          # a bf16 W^T needs 16-byte rows of dz
            got[form, lay] = run_bwdx(lib, cuda, c, D, prec, lay, form)
            compare(got[form, lay], want, f"{c['name']}/{form}/{lay}")
    for k, v in got.items():                                   # every form and layout: the same slabs in the same order
        same_bits(got["w", "a"], v, f"{c['name']} w/a against {k}")


# ------------------------------------------------------------------------------------------------------------------------
# grad-weight
# ------------------------------------------------------------------------------------------------------------------------
FORMS = {"f32": (R.F32, 32, False), "tr": (R.BF16, 64, False), "sh": (R.BF16, 64, True)}


def _r64(n):
    return (n + 63) // 64 * 64


def shadow(dev, values, rows):
    """bf16 copy as plan.py allocates shadows (rows to a multiple of 64, columns to one plus 64): rows past `rows` zero, the
    column padding of the live rows NaN (nothing may leak from it)"""
    v = np.asarray(values, dtype=np.float32)[:rows]
    s = torch.zeros((_r64(max(v.shape[0], 1)), _r64(v.shape[1]) + 64), dtype=torch.bfloat16, device=dev)
    s[:rows, v.shape[1]:] = float("nan")
    s[:rows, :v.shape[1]] = torch.from_numpy(bf16_round(v)).to(dev).to(torch.bfloat16)
    return s


class WLaunch:
    """the argument block of one grad-weight launch with its buffers"""

    def __init__(self, dev, c, D, form, lay, db_shift=0, ws_tail=16):
        from cdcmdr_amd import _lib as L
        self.c, self.a, self.keep, self.DW, self.DB = c, L.LinBwdwArgs(), [], [], []
        a = self.a
        a.n_groups, a.split_k, a.defer_reduce = len(c["groups"]), c["split"], c["defer"]
        self.stride = R.slab_layout(c)[1]
        self.ws = None
        if c["split"] > 1:
            self.ws = torch.full((c["split"] * self.stride + ws_tail,), float("nan"), device=dev)
            self.ws[c["split"] * self.stride:] = OUT_SENTINEL
            a.workspace = self.ws.data_ptr()
        if c["rows"] is not None:
            self.keep.append(i32(dev, R.offsets(c["rows"])))
            a.row_offsets = self.keep[-1].data_ptr()
        for g, (M, N, K, has_db, acc, extra) in enumerate(c["groups"]):
            rng = np.random.default_rng(g)
            DZ, X = buf(dev, D["dz"][g], lay), buf(dev, D["x"][g], lay)
            # a deferred launch must leave dw / db alone: they start from values, not NaN, so that the bits can be compared
            dw0 = D["dw0"][g] if (acc or c["defer"]) else nan_like(N, K)
            db0 = D["db0"][g] if (acc or c["defer"]) else nan_like(1, N)
            self.DW.append(buf(dev, dw0, lay, out=True, extra=extra))
            G = a.g[g]
            G.dz, G.lddz, G.x, G.ldx, G.dw, G.lddw = DZ.ptr, DZ.ld, X.ptr, X.ld, self.DW[g].ptr, self.DW[g].ld
            G.M = (c["M_arg"] or c["R"]) if c["rows"] is not None else M
            G.N, G.K, G.accumulate = N, K, acc
            self.DB.append(None)
            if has_db:
                shifted = np.concatenate([np.full(db_shift, OUT_SENTINEL, np.float32), np.asarray(db0, np.float32).ravel()])
                self.DB[g] = buf(dev, shifted, lay, out=True)
                G.db = self.DB[g].ptr + 4 * db_shift
            if form == "sh":
                dzh, xh = shadow(dev, D["dz"][g], M), shadow(dev, D["x"][g], M)
                G.dzh, G.lddzh, G.xh, G.ldxh = dzh.data_ptr(), dzh.stride(0), xh.data_ptr(), xh.stride(0)
                self.keep += [dzh, xh]
            self.keep += [DZ, X]
        self.db_shift = db_shift

    def results(self):
        out = {}
        for g, (M, N, K, has_db, *_r) in enumerate(self.c["groups"]):
            out[f"dw{g}"] = self.DW[g].read(f"dw{g}")
            if has_db:
                full = self.DB[g].read(f"db{g}")[0]
                assert (full[:self.db_shift] == OUT_SENTINEL).all()
                out[f"db{g}"] = full[self.db_shift:]
        return out

    def slabs(self):
        h = self.ws.cpu().numpy()
        n = self.c["split"] * self.stride
        assert (h[n:] == OUT_SENTINEL).all(), "wrote past the workspace"
        return h[:n].reshape(self.c["split"], self.stride)


def run_bwdw(lib, dev, c, D, form, lay, **kw):
    w = WLaunch(dev, c, D, form, lay, **kw)
    call(lib, "cdc_glinear_bwd_w", C.byref(w.a), FORMS[form][0])
    return w


def check_slabs(c, w, want, what):
    """every slice's slab, the empty ones included, where the header puts it"""
    sw, sb = R.slab_sums(c, want, want)
    got = w.slabs()
    ok = np.isfinite(sw)                                       # (the db piece of a group without db is not defined)
    assert_bounded(got[ok], sw[ok], sb[ok], f"{what} slabs")
    return got


def check_deferred(c, D, w, want, form, what):
    """dw / db bit-unchanged, the workspace holds the slabs in the documented layout, their float64 sum is within the bound"""
    prec, unit, rounded = FORMS[form]
    for g, (M, N, K, has_db, *_r) in enumerate(c["groups"]):
        assert_bits_equal(w.DW[g].read(), D["dw0"][g], f"{what}: dw{g} written by a deferred launch")
        if has_db:
            assert_bits_equal(w.DB[g].read()[0], D["db0"][g], f"{what}: db{g} written by a deferred launch")
    got = check_slabs(c, w, want, what)
    total =R.ref_bwdw(dict(c, defer=0), D, prec, unit, db_rounded=rounded)
    off, _ = R.slab_layout(c)
    tot = got.astype(np.float64).sum(0)
    for g, (M, N, K, has_db, *_r) in enumerate(c["groups"]):
        # the float64 sum of the fp32 slabs: each slab within its own bound, no rounding in between
        assert_bounded(tot[off[g][0]:off[g][0] + N * K].reshape(N, K), *total[f"dw{g}"], f"{what} sum of slabs dw{g}")
        if has_db:
            assert_bounded(tot[off[g][1]:off[g][1] + N], *total[f"db{g}"], f"{what} sum of slabs db{g}")


@pytest.mark.parametrize("form,i", [(f, i) for f in FORMS for i in range(len(R.bwdw_cases(f)))],
                         ids=[c["name"] for f in FORMS for c in R.bwdw_cases(f)])
def test_grad_weight(cuda, lib, form, i):
    c = R.bwdw_cases(form)[i]
    prec, unit, rounded = FORMS[form]
    D, want = ref("bwdw", c, prec, unit=unit, db_rounded=rounded)
    got = {}
    for lay in "am":
        w = run_bwdw(lib, cuda, c, D, form, lay)
        if c["defer"]:
            check_deferred(c, D, w, want, form, f"{c['name']}/{lay}")
            got[lay] = {"slabs": np.nan_to_num(w.slabs(), nan=0.0)}
        else:
            got[lay] = w.results()
            if c["split"] > 1:
                got[lay]["slabs"] = np.nan_to_num(check_slabs(c, w, want, f"{c['name']}/{lay}"), nan=0.0)
            compare(got[lay], {k: v for k, v in want.items() if not k.startswith("slab")}, f"{c['name']}/{lay}")
    same_bits(got["a"], got["m"], c["name"])


# ------------------------------------------------------------------------------------------------------------------------
# the reduce launch: the slabs of a deferred launch added on the host in fp32, in slice order from 0, then the old value
# ------------------------------------------------------------------------------------------------------------------------
REDUCE = {
    # 16-byte branch: everything aligned, lddw == K, every N K and every flat start a multiple of 4
    "vec4": ([(200, 8, 12, 1, 0, 0), (200, 4, 8, 1, 1, 0), (200, 4, 4, 1, 0, 0)], "a", 0),
    "vec4nodb": ([(200, 8, 12, 0, 0, 0), (200, 4, 8, 1, 1, 0), (200, 8, 4, 0, 1, 0)], "a", 0),
    # the issue's shape: the last group's N is not a multiple of 4 (the stride is then odd: the scalar branch, see the docstring)
    "lastN3": ([(200, 8, 12, 1, 0, 0), (200, 4, 8, 1, 1, 0), (200, 3, 8, 1, 0, 0)], "a", 0),
    "lddw": ([(200, 8, 12, 1, 0, 4), (200, 4, 8, 1, 1, 0)], "a", 0),
    "dboff4": ([(200, 8, 12, 1, 1, 0), (200, 4, 8, 1, 0, 0)], "a", 1),
    "odd": ([(200, 3, 5, 1, 1, 1), (200, 5, 7, 0, 0, 0), (200, 1, 1, 1, 0, 0)], "m", 0),
}


def host_reduce(slabs, old):
    s = np.zeros(slabs.shape[1:], np.float32)
    for k in range(slabs.shape[0]):
        s = s + slabs[k]
    return s if old is None else (np.asarray(old, np.float32) + s).astype(np.float32)


@pytest.mark.parametrize("form", ["f32", "sh"])
@pytest.mark.parametrize("split", [3, 4, 9])
@pytest.mark.parametrize("name", list(REDUCE))
def test_reduce_launch(cuda, lib, name, split, form):
    groups, lay, shift = REDUCE[name]
    c = R.bwdw_case(f"reduce_{name}", groups, split=split)
    D = R.make_data(c)
    plain = [tuple(g[:4]) + (0,) + tuple(g[5:]) for g in groups]     # the deferred launch may not accumulate
    slabs = run_bwdw(lib, cuda, dict(c, groups=plain, defer=1), D, form, lay, db_shift=shift).slabs()
    got = run_bwdw(lib, cuda, c, D, form, lay, db_shift=shift).results()
    off, _ = R.slab_layout(c)
    for g, (M, N, K, has_db, acc, _e) in enumerate(groups):
        want = host_reduce(slabs[:, off[g][0]:off[g][0] + N * K], D["dw0"][g].ravel() if acc else None)
        assert_bits_equal(got[f"dw{g}"].ravel(), want, f"{name} dw{g}")
        if has_db:
            assert_bits_equal(got[f"db{g}"], host_reduce(slabs[:, off[g][1]:off[g][1] + N], D["db0"][g] if acc else None), f"{name} db{g}")


# ------------------------------------------------------------------------------------------------------------------------
# the pair launches: a wide and a narrow block in one launch, bit-equal to two cdc_glinear_bwd_w calls
# ------------------------------------------------------------------------------------------------------------------------
WIDE = [(200, 129, 65, 1, 0, 0), (200, 64, 130, 1, 0, 2), (200, 130, 8, 0, 0, 0)]
NARROW = [(200, 64, 96, 1, 0, 0), (200, 3, 129, 1, 0, 1), (200, 5, 8, 0, 0, 0)]


def tabs(dev, wide, narrow):
    return torch.frombuffer(bytearray(bytes(wide.a) + bytes(narrow.a)), dtype=torch.uint8).to(dev)


def pair_blocks(dev, split, defer, acc=0):
    with_acc = lambda gs: [g[:4] + (acc if i == 0 else 0,) + g[5:] for i, g in enumerate(gs)]
    cw = R.bwdw_case("pair_wide", with_acc(WIDE), split=split[0], defer=defer if split[0] > 1 else 0)
    cn = R.bwdw_case("pair_narrow", with_acc(NARROW), split=split[1], defer=defer if split[1] > 1 else 0)
    return cw, R.make_data(cw), cn, R.make_data(cn)


@pytest.mark.parametrize("lay", ["a", "m"])
@pytest.mark.parametrize("split", [(1, 1), (3, 5), (1, 4), (2, 1)])
def test_pair_launch_equals_two_single_launches(cuda, lib, split, lay):
    cw, Dw, cn, Dn = pair_blocks(cuda, split, defer=1, acc=1 if split == (1, 1) else 0)
    single = [run_bwdw(lib, cuda, c, D, "sh", lay) for c, D in ((cw, Dw), (cn, Dn))]
    pair = [WLaunch(cuda, c, D, "sh", lay) for c, D in ((cw, Dw), (cn, Dn))]
    t = tabs(cuda, *pair)
    call(lib, "cdc_glinear_bwd_w_pair", C.byref(pair[0].a), C.byref(pair[1].a), C.c_void_p(t.data_ptr()))
    torch.cuda.synchronize()
    for one, two, c in zip(single, pair, (cw, cn)):
        same_bits(one.results(), two.results(), c["name"])             # a deferred block: both left untouched
        if c["split"] > 1:
            assert_bits_equal(np.nan_to_num(one.slabs()), np.nan_to_num(two.slabs()), f"{c['name']} slabs")
    for c, D, w in ((cw, Dw, pair[0]), (cn, Dn, pair[1])):                # and against float64
        want = R.ref_bwdw(c, D, R.BF16, 64, db_rounded=True)
        if c["defer"]:
            check_deferred(c, D, w, want, "sh", c["name"])
        else:
            compare(w.results(), want, c["name"])


@pytest.mark.parametrize("lay", ["a", "m"])
@pytest.mark.parametrize("split", [(3, 5), (4, 2)])
def test_pair_reduce_equals_two_split_launches(cuda, lib, split, lay):
    cw, Dw, cn, Dn = pair_blocks(cuda, split, defer=0)
    single = [run_bwdw(lib, cuda, c, D, "sh", lay) for c, D in ((cw, Dw), (cn, Dn))]
    # the pair's blocks are deferred (its reduce is a launch of its own); their dw / db start from values that must all go
    pair = [WLaunch(cuda, dict(c, defer=1), D, "sh", lay) for c, D in ((cw, Dw), (cn, Dn))]
    t = tabs(cuda, *pair)
    call(lib, "cdc_glinear_bwd_w_pair_reduce", C.byref(pair[0].a), C.byref(pair[1].a), C.c_void_p(t.data_ptr()))
    torch.cuda.synchronize()
    for one, two, c, D in zip(single, pair, (cw, cn), (Dw, Dn)):
        same_bits(one.results(), two.results(), c["name"])
        assert_bits_equal(np.nan_to_num(one.slabs()), np.nan_to_num(two.slabs()), f"{c['name']} slabs")
        want = R.ref_bwdw(c, D, R.BF16, 64, db_rounded=True)
        compare(two.results(), {k: v for k, v in want.items() if not k.startswith("slab")}, c["name"])


# ------------------------------------------------------------------------------------------------------------------------
# cdc_transpose_multi
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
def test_transpose_multi(cuda, lib, half):
    from cdcmdr_amd import _lib as L
    rng = np.random.default_rng(7)
    shapes = [(1, 1), (1, 65), (31, 33), (32, 32), (33, 31), (65, 1), (65, 65), (32, 1), (33, 65)]
    mats = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    # values exactly between two bf16 numbers (ties to even, both ways), NaN, infinities, the largest finite value, denormals
    special = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7FC00000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000001,
                        0x00008000, 0x3F807FFF, 0x3F808001], dtype=np.uint32).view(np.float32)
    mats[6].ravel()[:special.size] = special
    mats[2].ravel()[-special.size:] = special
    ta, src, dst, tail = L.TransposeArgs(), [], [], 8
    ta.n = len(mats)
    for i, m in enumerate(mats):
        src.append(torch.from_numpy(m).to(cuda))
        if half:
            d = torch.full((m.size + tail,), -3.0, dtype=torch.bfloat16, device=cuda)
            ta.bf16_mask |= 1 << i
        else:
            d = torch.full((m.size + tail,), OUT_SENTINEL, device=cuda)
        dst.append(d)
        ta.t[i].src, ta.t[i].dst, ta.t[i].rows, ta.t[i].cols = src[i].data_ptr(), d.data_ptr(), m.shape[0], m.shape[1]
    call(lib, "cdc_transpose_multi", C.byref(ta))
    for m, d in zip(mats, dst):
        if half:
            h = d.view(torch.int16).cpu().numpy().view(np.uint16)
            want = bf16_bits(m.T)
            got = h[:m.size].reshape(m.T.shape)
            nan = np.isnan(m.T)
            assert np.array_equal(got[~nan], want[~nan]), f"{m.shape}: not the round-to-nearest-even bf16"
            assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x007F) != 0).all(), "NaN did not stay NaN"
            assert (h[m.size:] == 0xC040).all(), f"{m.shape}: wrote past rows x cols"
        else:
            h = d.cpu().numpy()
            assert np.array_equal(h[:m.size].reshape(m.T.shape).view(np.int32), np.ascontiguousarray(m.T).view(np.int32)), f"{m.shape}"
            assert (h[m.size:] == OUT_SENTINEL).all(), f"{m.shape}: wrote past rows x cols"


# ------------------------------------------------------------------------------------------------------------------------
# the 128 x 128 class: the launcher counts tiles from M, an upper bound under row_offsets — 32 ragged groups with M = 65536
# and N <= 64 are 32768 counted 64 x 64 tiles (>= 16384) on a few hundred real rows
# ------------------------------------------------------------------------------------------------------------------------
BIG_ROWS = tuple((130, 1, 0, 65, 7, 64, 129, 3)[g % 8] for g in range(32))
BIG_M = 65536


@pytest.mark.parametrize("prec", PRECS)
def test_forward_128_class(cuda, lib, prec):
    c = R.fwd_case("big_f", 40, None, [(64, 3, 33, 1)[g % 4] for g in range(32)], act=[(0, 2, 33, 1)[g % 4] for g in range(32)],
                   bias=[g % 3 != 0 for g in range(32)], rows=BIG_ROWS, p=0.2, step=3)
    assert sum(-(-BIG_M // 64) * -(-n // 64) for n in c["Ns"]) >= 16384
    D, want = ref("fwd", c, prec)
    big = {lay: run_fwd(lib, cuda, c, D, prec, lay, M_arg=BIG_M) for lay in "am"}
    small = run_fwd(lib, cuda, c, D, prec, "a", M_arg=int(sum(BIG_ROWS)))       # 32 x 8 counted tiles: the 64 x 64 class
    for lay in "am":
        compare(big[lay], want, f"big_f/{lay}")
        same_bits(big[lay], small, f"big_f/{lay} against the 64 x 64 class")


@pytest.mark.parametrize("prec,form", [(R.BF16, "w"), (R.BF16, "wt"), (R.BF16, "wth"), (R.F32, "w"), (R.F32, "wt")],
                         ids=["bf16-w", "bf16-wt", "bf16-wth", "f32-w", "f32-wt"])
def test_grad_input_128_class(cuda, lib, prec, form):
    Ks = [(64, 3, 33, 1)[o % 4] for o in range(32)]
    c = R.bwdx_case("big_x", None, [(K, (None, K - 1, K)[o % 3], o % 2) for o, K in enumerate(Ks)], [((40, 8, 64, 96)[s % 4], s) for s in range(32)],
                    mask_scale=1.25, rows=BIG_ROWS)
    assert sum(-(-BIG_M // 64) * -(-K // 64) for K in Ks) >= 16384
    D, want = ref("bwdx", c, prec)
    lays = "a" if form == "wth" else "am"                      # a bf16 W^T needs 16-byte rows of dz
    big = {lay: run_bwdx(lib, cuda, c, D, prec, lay, form, M_arg=BIG_M) for lay in lays}
    small = run_bwdx(lib, cuda, c, D, prec, "a", form, M_arg=int(sum(BIG_ROWS)))
    plain = run_bwdx(lib, cuda, c, D, prec, "a", "w", M_arg=int(sum(BIG_ROWS)))
    for lay in lays:
        compare(big[lay], want, f"big_x/{form}/{lay}")
        same_bits(big[lay], small, f"big_x/{form}/{lay} against the 64 x 64 class")
        same_bits(big[lay], plain, f"big_x/{form}/{lay} against w in the 64 x 64 class")


def test_forward_128_class_dense_production_shape(cuda, lib):
    """M = 32768, K = 40, N = 2048 over five groups, bf16: 512 x 32 = 16384 counted tiles.  Sampled rows against float64, every
    row bit for bit against two launches of 16384 rows each (8192 tiles: the 64 x 64 class)."""
    from cdcmdr_amd import _lib as L
    M, K, Ns = 32768, 40, [1024, 512, 256, 192, 64]
    rng = np.random.default_rng(11)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1))
    w = [(rng.standard_normal((n, K)) / K ** 0.5).astype(np.float32) for n in Ns]
    b = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in Ns]
    xd, wd, bd = x.to(cuda), [torch.from_numpy(v).to(cuda) for v in w], [torch.from_numpy(v).to(cuda) for v in b]
    ld = sum(Ns) + 4
    ys = [torch.full((M, ld), float("nan"), device=cuda) for _ in range(2)]

    def launch(y, r0, rows):
        a = L.LinFwdArgs()
        a.n_groups, a.relu = len(Ns), 1
        col = 0
        for g, n in enumerate(Ns):
            G = a.g[g]
            G.x, G.ldx, G.w, G.ldw, G.bias = xd.data_ptr() + 4 * r0 * K, K, wd[g].data_ptr(), K, bd[g].data_ptr()
            G.y, G.ldy, G.M, G.N, G.K, G.act_cols = y.data_ptr() + 4 * (r0 * ld + col), ld, rows, n, K, n - 3
            col += n
        call(lib, "cdc_glinear_fwd", C.byref(a), R.BF16)

    launch(ys[0], 0, M)
    launch(ys[1], 0, M // 2)
    launch(ys[1], M // 2, M // 2)
    assert bool(torch.isnan(ys[0][:, sum(Ns):]).all()), "wrote past the N columns"
    assert torch.equal(ys[0][:, :sum(Ns)], ys[1][:, :sum(Ns)]), "128 x 128 class differs from the 64 x 64 class"
    rows = np.unique(np.r_[0:130, np.arange(0, M, 257), M - 130:M])
    got = ys[0][torch.from_numpy(rows).to(cuda)].cpu().numpy()
    c = R.fwd_case("dense", K, len(rows), Ns, act=[n - 3 for n in Ns])
    want = R.ref_fwd(c, dict(x=x.numpy()[rows], w=w, b=b), R.BF16)
    col = 0
    for g, n in enumerate(Ns):
        assert_bounded(got[:, col:col + n], *want[f"y{g}"], f"dense y{g}")
        col += n


# ------------------------------------------------------------------------------------------------------------------------
# argument checks: an error before any launch
# ------------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, text):
    msg = lib.cdc_last_error() or b""
    assert rc < 0 and text.encode() in msg, (rc, msg)


def test_grad_input_argument_checks(cuda, lib):
    from cdcmdr_amd import _lib as L
    t = torch.zeros(64 * 64 + 8, device=cuda)
    h = torch.zeros(64 * 64 + 16, dtype=torch.bfloat16, device=cuda)

    def args(n_seg=1):
        a = L.LinBwdxArgs()
        a.n_out, a.n_seg, a.mask_scale = 1, n_seg, 1.0
        a.o[0].dx, a.o[0].lddx, a.o[0].M, a.o[0].K = t.data_ptr(), 16, 4, 16
        for s in range(n_seg):
            S = a.s[s]
            S.dz, S.lddz, S.w, S.ldw, S.N, S.out = t.data_ptr(), 16, t.data_ptr(), 16, 16, 0
            S.wt, S.ldwt, S.wt_bf16 = h.data_ptr(), 16, 1
        return a

    before = t.clone()
    a = args()
    _refused(lib, lib.cdc_glinear_bwd_x(C.byref(a), R.F32, _stream()), "bf16 transposed copy not eligible")
    a = args()
    a.s[0].ldwt = 20
    _refused(lib, lib.cdc_glinear_bwd_x(C.byref(a), R.BF16, _stream()), "bf16 transposed copy not eligible")
    a = args()
    a.s[0].wt = h.data_ptr() + 2
    _refused(lib, lib.cdc_glinear_bwd_x(C.byref(a), R.BF16, _stream()), "bf16 transposed copy not eligible")
    a = args(2)
    a.s[1].wt, a.s[1].wt_bf16 = None, 0
    _refused(lib, lib.cdc_glinear_bwd_x(C.byref(a), R.BF16, _stream()), "need every segment transposed")
    torch.cuda.synchronize()
    assert torch.equal(t, before), "a refused launch wrote"


def test_grad_weight_argument_checks(cuda, lib):
    c = R.bwdw_case("args", [(65, 8, 12, 1, 0, 0)], split=2)
    D = R.make_data(c)
    w = WLaunch(cuda, c, D, "f32", "a")
    w.a.workspace = None
    _refused(lib, lib.cdc_glinear_bwd_w(C.byref(w.a), R.F32, _stream()), "split_k needs a workspace")
    w = WLaunch(cuda, c, D, "f32", "a")
    w.a.split_k = 257
    _refused(lib, lib.cdc_glinear_bwd_w(C.byref(w.a), R.F32, _stream()), "split_k too large")
    w = WLaunch(cuda, dict(c, defer=1), D, "f32", "a")
    w.a.g[0].accumulate = 1
    _refused(lib, lib.cdc_glinear_bwd_w(C.byref(w.a), R.F32, _stream()), "cannot be left to the consumer")
    torch.cuda.synchronize()
    assert np.isnan(w.slabs()).all(), "a refused launch wrote"


def test_pair_argument_checks(cuda, lib):
    def blocks(split=(1, 1), defer=1):
        cw, Dw, cn, Dn = pair_blocks(cuda, split, defer=defer)
        return [WLaunch(cuda, c, D, "sh", "a") for c, D in ((cw, Dw), (cn, Dn))]

    def pair(p, fn="cdc_glinear_bwd_w_pair"):
        t = tabs(cuda, *p)
        return getattr(lib, fn)(C.byref(p[0].a), C.byref(p[1].a), C.c_void_p(t.data_ptr()), _stream())

    def untouched(p):
        torch.cuda.synchronize()
        for w in p:
            for g, DW in enumerate(w.DW):
                assert np.array_equal(DW.t.cpu().numpy().view(np.int32), DW.host0.view(np.int32)), "a refused launch wrote"
            if w.ws is not None:
                assert np.isnan(w.slabs()).all(), "a refused launch wrote slabs"

    p = blocks()
    ro = i32(cuda, [0, 200, 200, 200])
    p[1].a.row_offsets = ro.data_ptr()
    _refused(lib, pair(p), "ragged rows")
    untouched(p)
    p = blocks()
    p[1].a.g[0].N = 65
    _refused(lib, pair(p), "narrow class has 65 output rows")
    untouched(p)
    p = blocks(split=(3, 1), defer=1)
    p[0].a.defer_reduce = 0
    _refused(lib, pair(p), "leaves its slabs to the consumer")
    untouched(p)
    p = blocks()
    p[0].a.g[1].xh = None
    _refused(lib, pair(p), "bf16 shadows")
    untouched(p)
    # the reduce form needs both classes split, and says so before anything is launched
    for split in ((3, 1), (1, 3), (1, 1)):
        p = blocks(split=split, defer=1)
        _refused(lib, pair(p, "cdc_glinear_bwd_w_pair_reduce"), "both classes must be split")
        untouched(p)
