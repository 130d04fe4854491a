"""float64 restatement of what include/cdcmdr.h promises for cdc_gemm_bf16_nt (both modes, the BatchNorm partial sums included),
every value with a DERIVED error bound, the forward's 16-bit dropout stream, the seeded defects the bounds have to reject, the
launcher's tile choice restated, and the launches tests/test_gpu_gemm2_direct.py runs.  No GPU: tests/test_gemm2_ref_cpu.py holds
this file, tests/test_gpu_gemm2_direct.py holds the launches to it.

A launch is a case (see `case` / `out`): outputs o with M, N, what is written (y, yh), the epilogue's switches, and segments
(K, out[, operand]) in launch order; out_o = epilogue(sum over its segments of A_s[M, K_s] . B_s[N, K_s]^T).  Operands ARE bf16
(make_data rounds them); the contraction runs in float64 over the true K, cut into the kernel's 64-wide slabs only so that the
ring defects can be seeded (the K padding contributes nothing).  ref returns name -> (want, bound):
  y<o>     the fp32 output;  yh<o>  the bf16 output of an output WITHOUT y (with y, yh is the bf16 rounding of the y that was
           written: a bit equality, `check`);  bn1_<o> / bn2_<o>  the [64-row block, column] sums of y and y^2.

The bounds, as tests/glinear_ref.py: an element is a sum of n exact products and c further fp32 roundings,
sum_bound(sum |a_i b_i|, n, c), with
  * forward:    n = the output's K (all its segments); c = 1 with a bias, + 1 for the dropout scale (1 / (1 - p) taken as the fp32
                value the kernel computes); a dropped element is 0 exactly (bound 0);
  * grad-input: n = the sum of the segments' N; c = 1 for mask_scale, + 1 for the += (|old| joins the terms); a masked
                element is 0 exactly;
  * capped by glinear_ref.Y_FIG (forward) / G_FIG (grad-input): no new tolerance;
  * yh alone: the bound of y plus half a bf16 ulp at |y| + bound;
  * partial sums: double sums of the fp32 y the kernel formed: the rows' y bounds summed; squares 2 |y| b + b^2 summed; both plus
    rows 2^-53 sum |term| for the double additions."""
import numpy as np

from bn_ref import bf16_bits, bf16_from_bits, bf16_half_ulp, bf16_round, keep_mask_bits16
from glinear_ref import G_FIG, Y_FIG
from helpers import assert_bounded, capped, sum_bound

SEED = 0x0BAD_5EED_1234_5678
U53 = 2.0 ** -53
BK = 64
MAX_OUT, MAX_SEG = 24, 32
CLASSES = {1: (128, 128, 2), 2: (128, 128, 3), 3: (128, 128, 4), 4: (64, 128, 3), 5: (64, 128, 4), 6: (128, 64, 2), 7: (128, 64, 3),
           8: (64, 64, 4), 9: (64, 64, 3), 10: (64, 128, 2)}            # tile_cfg -> (BM, BN, ring depth), csrc/gemm2.hip
f64 = lambda a: np.asarray(a, dtype=np.float64)
f32 = lambda a: np.asarray(a, dtype=np.float32)

DEFECTS = ("k_tail", "seg_omitted", "slab_twice", "slab_skipped", "stale_slab", "next_seg_first_slab_lost", "no_bias", "relu_extra_col",
           "mask_extra_col", "no_mask_scale", "acc_off", "drop_halves_swapped", "drop_tile_local_row", "stream_id_ignored", "step_ignored",
           "yh_truncated", "bn_last_row_dropped", "bn_bias_omitted")


def r64(n):
    return (n + 63) // 64 * 64


def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


# ------------------------------------------------------------------------------------------------------------------------
# launch descriptions
# ------------------------------------------------------------------------------------------------------------------------
def out(M, N, bias=False, act=0, kind="y", acc=0, mask=None, sid=0, bn=None):
    """kind: "y", "h" (yh only) or "yh" (both); mask: None, "f" (fp32) or "h" (bf16); bn: None or bn_col0"""
    assert kind in ("y", "h", "yh") and mask in (None, "f", "h") and not (acc and kind == "h")
    return dict(M=M, N=N, bias=bias, act=act, kind=kind, acc=acc, mask=mask, sid=sid, bn=bn)


def case(name, mode, outs, segs, relu=1, p=0.0, step=None, mask_scale=1.0, bn_total=0, expect=None):
    """segs: (K, out) or (K, out, operand) in launch order: segments naming the same operand share A and B (their outputs have the
    same M and N).  expect: the tile class the library must choose by itself (auto_class)."""
    segs = [tuple(s) + ((i,) if len(s) == 2 else ()) for i, s in enumerate(segs)]
    assert 0 < len(outs) <= MAX_OUT and 0 < len(segs) <= MAX_SEG and all(0 <= s[1] < len(outs) for s in segs)
    return dict(name=name, mode=mode, outs=outs, segs=segs, relu=relu, p=p, step=step, mask_scale=mask_scale, bn_total=bn_total,
                expect=expect)


def out_segs(c, o):
    return [(s, K, op) for s, (K, so, op) in enumerate(c["segs"]) if so == o]


def slab_counts(c, o):
    return [r64(K) // BK for _, K, _ in out_segs(c, o)]


def auto_class(c):
    """the launcher's own choice (tile_cfg = 0), restated from csrc/gemm2.hip"""
    tiles = lambda bm, bn: sum(-(-O["M"] // bm) * -(-O["N"] // bn) for O in c["outs"])
    narrow = max(O["N"] for O in c["outs"]) <= 64
    short_rows = tiles(128, 64 if narrow else 128) < 256
    max_kr = max(sum(r64(K) for _, K, _ in out_segs(c, o)) for o in range(len(c["outs"])))
    if narrow:
        return 9 if short_rows else 7
    if short_rows:
        return 9 if max_kr >= 1024 else 10
    return 1


def keep_scale(p):
    return float(np.float32(1) / (np.float32(1) - np.float32(p))) if p > 0 else 1.0


def keep(c, o, defect=None):
    """the keep mask [M, N] of output o"""
    O = c["outs"][o]
    rows = np.arange(O["M"])
    if defect == "drop_tile_local_row":
        rows = rows % 64
    sid = 0 if defect == "stream_id_ignored" else O["sid"]
    step = None if defect == "step_ignored" else c["step"]
    N2 = O["N"] + (O["N"] & 1)
    k = keep_mask_bits16(SEED, step, sid - 64, rows, N2, c["p"])
    if defect == "drop_halves_swapped":
        k = k[:, np.arange(N2) ^ 1]
    return k[:, :O["N"]]


# ------------------------------------------------------------------------------------------------------------------------
# data: operands bf16-rounded, a ~ N(0, 1), b ~ N(0, 1) / sqrt(the output's reduction length)
# ------------------------------------------------------------------------------------------------------------------------
MASK_SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x0080, 0x8001, 0xBF80], dtype=np.uint16)   # +0, -0, the smallest positive bf16
#                                                                         (subnormal), the smallest normal, negative values


def make_data(c):
    rng = _rng(c["name"])
    n = lambda *s, scale=1.0: f32(scale * rng.standard_normal(s))
    D = dict(a={}, b={}, bias=[], mask=[], y0=[])
    for o, O in enumerate(c["outs"]):
        ktot = sum(K for _, K, _ in out_segs(c, o))
        for _, K, op in out_segs(c, o):
            if op in D["a"]:
                assert D["a"][op].shape == (max(O["M"], 1), K) and D["b"][op].shape == (O["N"], K), "shared operands: same M, N, K"
                continue
            D["a"][op], D["b"][op] = bf16_round(n(max(O["M"], 1), K)), bf16_round(n(O["N"], K, scale=max(ktot, 1) ** -0.5))
        D["bias"].append(n(O["N"], scale=0.3))
        m = bf16_round(n(O["M"], O["N"]))
        special = rng.random(m.shape) < 0.3
        m[special] = bf16_from_bits(rng.choice(MASK_SPECIALS, int(special.sum())))
        D["mask"].append(m)
        D["y0"].append(n(O["M"], O["N"]))
    return D


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def _slabs(c, D, o, defect):
    """[(segment position, slab, product, sum |a||b|)] of output o in the order the ring runs them"""
    O, S = c["outs"][o], []
    for pos, (s, K, op) in enumerate(out_segs(c, o)):
        if defect == "seg_omitted" and s == len(c["segs"]) - 1:
            continue
        a, b = np.zeros((O["M"], r64(K))), np.zeros((O["N"], r64(K)))
        a[:, :K], b[:, :K] = f64(bf16_round(D["a"][op]))[:O["M"]], f64(bf16_round(D["b"][op]))
        if defect == "k_tail":
            a[:, K - 1] = 0.0
        nk = r64(K) // BK
        for t in range(nk):
            if (defect == "slab_skipped" and pos == 0 and t == nk - 1) or (defect == "next_seg_first_slab_lost" and pos > 0 and t == 0):
                continue
            at, bt = a[:, t * BK:(t + 1) * BK], b[:, t * BK:(t + 1) * BK]
            S.append([at @ bt.T, np.abs(at) @ np.abs(bt).T])
            if defect == "slab_twice" and pos == 0 and t == 0:
                S.append(S[-1])
    if defect == "stale_slab" and len(S) >= 2:
        S[-1] = S[-2]
    return S


def ref(c, D, defect=None, as_kernel=False):
    """name -> (want, bound); as_kernel: name -> what a kernel that rounds each float64 result ONCE would leave (y in fp32, yh its
    bf16 rounding, the partial sums double sums of that fp32 y) — the values the bounds must accept, and with a defect reject"""
    res = {}
    fwd = c["mode"] == 0
    ms = 1.0 if defect == "no_mask_scale" else float(np.float32(c["mask_scale"]))
    for o, O in enumerate(c["outs"]):
        M, N = O["M"], O["N"]
        v, t = np.zeros((M, N)), np.zeros((M, N))
        for p_, t_ in _slabs(c, D, o, defect):
            v, t = v + p_, t + t_
        n = max(sum(K for _, K, _ in out_segs(c, o)), 1)
        n_round = 0
        a = min(max(O["act"], 0) + (1 if defect == ("relu_extra_col" if fwd else "mask_extra_col") and 0 <= O["act"] < N else 0), N)
        pre_bias = v.copy()
        if fwd:
            if O["bias"] and defect != "no_bias":
                v, t, n_round = v + f64(D["bias"][o]), t + np.abs(f64(D["bias"][o])), 1
            bound = sum_bound(t, n, n_round)
            if a > 0 and c["relu"]:
                v[:, :a] = np.maximum(v[:, :a], 0.0)
            if a > 0 and c["p"] > 0:
                k, ks = keep(c, o, defect)[:, :a], keep_scale(c["p"])
                v[:, :a] = np.where(k, v[:, :a] * ks, 0.0)
                bound[:, :a] = np.where(k, sum_bound(t[:, :a] * ks, n, n_round + 1), 0.0)
            bound = capped(bound, v, Y_FIG)
        else:
            if O["mask"] is not None and a > 0:
                on = f64(D["mask"][o])[:, :a] > 0
                v[:, :a], t[:, :a], n_round = np.where(on, v[:, :a] * ms, 0.0), np.where(on, t[:, :a] * abs(ms), 0.0), 1
            if O["acc"] and defect != "acc_off":
                old = f64(D["y0"][o])
                v, t, n_round = v + old, t + np.abs(old), n_round + 1
            bound = capped(sum_bound(t, n, n_round), v, G_FIG)
        y32 = v.astype(np.float32)
        if "y" in O["kind"]:
            res[f"y{o}"] = y32 if as_kernel else (v, bound)
        if "h" in O["kind"]:
            if as_kernel:
                bits = (y32.view(np.uint32) >> 16).astype(np.uint16) if defect == "yh_truncated" else bf16_bits(y32)
                res[f"yh{o}"] = bf16_from_bits(bits).reshape(M, N)
            elif O["kind"] == "h":
                res[f"yh{o}"] = (v, np.where(bound == 0, 0.0, bound + bf16_half_ulp(np.abs(v) + bound)))
        if O["bn"] is not None:
            assert fwd and O["act"] == 0
            src = f64(y32) if as_kernel else v
            b = np.zeros_like(bound) if as_kernel else bound
            if defect == "bn_bias_omitted":
                src = pre_bias
            blocks = -(-M // 64)
            s1, s2, b1, b2 = (np.zeros((blocks, N)) for _ in range(4))
            for k in range(blocks):
                hi = min(64 * k + 64, M) - (1 if defect == "bn_last_row_dropped" and 64 * k + 64 >= M else 0)
                x, e = src[64 * k:hi], b[64 * k:hi]
                s1[k], s2[k] = x.sum(0), (x * x).sum(0)
                b1[k] = e.sum(0) + len(x) * U53 * np.abs(x).sum(0)
                b2[k] = (2 * np.abs(x) * e + e * e).sum(0) + len(x) * U53 * (x * x).sum(0)
            res[f"bn1_{o}"], res[f"bn2_{o}"] = (s1, s2) if as_kernel else ((s1, b1), (s2, b2))
    return res


def check(c, got, W, what):
    """every value within its bound; yh beside y: the round-to-nearest-even bf16 of the y that was written, bit for bit"""
    for k, (want, bound) in W.items():
        assert k in got, f"{what}: {k} not produced"
        assert_bounded(got[k], want, bound, f"{what} {k}")
    for o, O in enumerate(c["outs"]):
        if O["kind"] == "yh":
            assert np.array_equal(bf16_bits(got[f"yh{o}"]), bf16_bits(got[f"y{o}"])), f"{what}: yh{o} is not the bf16 rounding of y{o}"


# ------------------------------------------------------------------------------------------------------------------------
# memory layouts of the GPU launches, and the argument block (device pointers come from `ptr`)
# ------------------------------------------------------------------------------------------------------------------------
def layout(c, lay):
    """per output the row strides and the base offset (elements) of y, yh and the mask.
    "a": every pointer 16-byte aligned, ldy % 4 == 0, ldyh % 8 == 0, the mask likewise: the eight-column path wherever a piece is
    inside N and on one side of act_cols.  "m": ldy = N + 3, an odd ldyh pad and every base one element off the 16-byte grid: the
    element-wise path everywhere."""
    L = []
    for O in c["outs"]:
        N = O["N"]
        if lay == "a":
            L.append(dict(off=0, ldy=N + (-N) % 4 + 4, ldyh=N + (-N) % 8 + 8, ldmask=(N + (-N) % 8 + 8) if O["mask"] == "h" else N + (-N) % 4 + 4))
        else:
            L.append(dict(off=1, ldy=N + 3, ldyh=1 + N + (9 if (1 + N + 9) % 8 else 11), ldmask=N + 3))
    return L


def fill_args(a, c, lay, ptr, tile_cfg=0):
    """a: cdcmdr_amd._lib.G2Args.  ptr(kind, index) -> address of "y" / "yh" / "mask" / "bias" (per output, the FIRST element of the
    allocation: the layout's offset is added here), "a" / "b" (per operand), "bn" and "step" (the launch's)."""
    L = layout(c, lay)
    a.n_out, a.n_seg, a.mode, a.relu, a.drop_p, a.mask_scale = len(c["outs"]), len(c["segs"]), c["mode"], c["relu"], c["p"], c["mask_scale"]
    a.tile_cfg, a.seed = tile_cfg, SEED
    a.seed_offset_dev = ptr("step", 0) if c["step"] is not None else None
    for o, (O, Lo) in enumerate(zip(c["outs"], L)):
        G = a.o[o]
        if "y" in O["kind"]:
            G.y, G.ldy = ptr("y", o) + 4 * Lo["off"], Lo["ldy"]
        if "h" in O["kind"]:
            G.yh, G.ldyh = ptr("yh", o) + 2 * Lo["off"], Lo["ldyh"]
        if O["bias"]:
            G.bias = ptr("bias", o)
        if O["mask"] is not None:
            G.mask, G.ldmask, G.mask_bf16 = ptr("mask", o) + (2 if O["mask"] == "h" else 4) * Lo["off"], Lo["ldmask"], int(O["mask"] == "h")
        if O["bn"] is not None:
            G.bn_partial, G.bn_col0, G.bn_total_c = ptr("bn", 0), O["bn"], c["bn_total"]
        G.M, G.N, G.act_cols, G.accumulate, G.stream_id = O["M"], O["N"], O["act"], O["acc"], O["sid"]
    for s, (K, o, op) in enumerate(c["segs"]):
        S = a.s[s]
        S.a, S.lda, S.b, S.ldb, S.Kr, S.out = ptr("a", op), r64(K) + 8, ptr("b", op), r64(K) + 8, r64(K), o
    return a


# ------------------------------------------------------------------------------------------------------------------------
# the launches tests/test_gpu_gemm2_direct.py runs and tests/test_gemm2_ref_cpu.py seeds the defects at
# ------------------------------------------------------------------------------------------------------------------------
KINDS = ("yh", "y", "h")
GEO_M, GEO_N = (1, 63, 64, 65, 129, 257), (5, 8, 64, 65, 72, 129, 136)


def geometry_cases():
    """forward, K = 100 (two slabs, 28 columns of K padding): per (M, bias) one launch of 21 outputs, N x act_cols in {0, N, 36}
    (36: a boundary inside an eight-column piece; beyond N for N = 5, 8: every column is activated)"""
    S = []
    for M in GEO_M:
        for bias in (True, False):
            outs = [out(M, N, bias=bias, act=act, kind=KINDS[(i + j + M) % 3], sid=i)
                    for i, N in enumerate(GEO_N) for j, act in enumerate((0, N, 36))]
            S.append(case(f"geo_M{M}_{'b' if bias else 'nb'}", 0, outs, [(100, o) for o in range(len(outs))]))
    return S


RING_K = (8, 100, 192, 256, 320, 448)                      # 1, 2, 3, 4, 5 and 7 slabs


def ring_case():
    """M = 65, N = 72: totals below the ring depth, both wait branches at depths 3 and 4"""
    return case("ring", 0, [out(65, 72, bias=True, act=36, kind="yh", sid=o) for o in range(len(RING_K))], [(K, o) for o, K in enumerate(RING_K)])


def segment_cases():
    seg32 = [((60, 128, 130)[(s // 3 + s % 3) % 3], s % 3) for s in range(32)]          # Kr cycles through 64, 128, 192
    return [
        case("seg_one", 1, [out(65, 96, act=86, mask="f", kind="yh")], [(100, 0)], mask_scale=1.25),
        case("seg_three", 1, [out(65, 96, act=86, mask="h", kind="yh", acc=1)], [(40, 0), (100, 0), (64, 0)], mask_scale=1.25),
        case("seg_32", 1, [out(65, 7, act=3, mask="f", kind="y"), out(65, 96, act=96, mask="h", kind="yh"), out(65, 136, kind="h")], seg32,
             mask_scale=1.25),
        case("seg_five", 1, [out(129, 72, act=62, mask="h", kind="y", acc=1)], [(64, 0)] * 5, mask_scale=1.25),
    ]


def gradin_cases():
    """per (M, width): one launch of 24 outputs = mask kind x act_cols x accumulate over ONE pair of operands; which of y / yh is
    written rotates (yh alone cannot accumulate: y then).  M = 65 in a 128-row class: prefetch passes beyond row_end."""
    S = []
    for ci, (M, W) in enumerate((M, W) for M in (1, 65, 129) for W in (7, 96, 136)):
        outs = []
        for mask in (None, "f", "h"):
            for act in (0, W, max(W - 10, 0), 3):
                for acc in (0, 1):
                    kind = KINDS[(len(outs) + ci) % 3]
                    outs.append(out(M, W, act=act, mask=mask, acc=acc, kind="y" if (kind == "h" and acc) else kind))
        S.append(case(f"gi_M{M}_W{W}", 1, outs, [(100, o, 0) for o in range(24)], mask_scale=1.25))
    return S


def many_cases():
    """24 outputs in one forward launch: M in {0, 1, 65, 200} mixed, different N, distinct stream ids, half of them yh only"""
    S = []
    for p, step, relu in ((0.5, 77, 1), (0.5, None, 0), (0.2, 70000, 0), (0.2, None, 1)):
        outs = []
        for i in range(24):
            N = (5, 8, 64, 65, 72, 129, 136, 33)[(i * 3) % 8]
            outs.append(out((65, 0, 200, 1)[i % 4], N, bias=i % 3 != 0, act=(N, N, max(N - 5, 1), 36)[(i // 4) % 4],
                            kind="h" if i % 2 else ("yh" if i % 4 else "y"), sid=5 * i + 1))
        S.append(case(f"many_p{p}_{'null' if step is None else step}", 0, outs, [(100, o) for o in range(24)], relu=relu, p=p, step=step))
    return S


def bn_case():
    """two outputs into one workspace of 144 columns at bn_col0 = 3 and 75; M = 257: five blocks, the last of one row"""
    return case("bn", 0, [out(257, 70, bias=True, kind="yh", bn=3), out(257, 64, bias=True, kind="y", bn=75)], [(100, 0), (72, 1)], bn_total=144)


def auto_cases():
    """launches whose counted tiles put the library's own choice in each branch of the selection"""
    mk = lambda name, n_out, M, N, K, expect: case(name, 0, [out(M, N, bias=True, act=N // 2, kind="yh", sid=o) for o in range(n_out)],
                                                   [(K, o, 0) for o in range(n_out)], expect=expect)
    return [mk("auto_1", 24, 1281, 65, 64, 1), mk("auto_7", 24, 1281, 64, 64, 7), mk("auto_9", 1, 65, 264, 1024, 9), mk("auto_10", 1, 65, 264, 100, 10)]


def dropout_cases():
    return many_cases()


def all_cases():
    return geometry_cases() + [ring_case()] + segment_cases() + gradin_cases() + many_cases() + [bn_case()] + auto_cases()
