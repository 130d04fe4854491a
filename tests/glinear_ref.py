"""float64 restatement of what include/cdcmdr.h promises for cdc_glinear_fwd, cdc_glinear_bwd_x and cdc_glinear_bwd_w (the split
launch's slabs included), every value with a DERIVED error bound, the forward's dropout stream, the seeded defects the bounds have
to reject, and the launches tests/test_gpu_glinear.py runs.  No GPU: tests/test_glinear_ref_cpu.py holds this file,
tests/test_gpu_glinear.py holds the launches to it.

Every ref_* function returns name -> (want, bound).  A case is a dict (fwd_case / bwdx_case / bwdw_case); its data comes from
make_data, seeded by the case's name.

The bounds.  An output element is a sum of n products and c further fp32 roundings: sum_bound(sum |a_i b_i|, n, c), where
  * forward:     n = K; c = 1 with a bias, + 1 for the dropout scale (1 / (1 - p) is taken as the fp32 value the kernel computes);
  * grad-input:  n = sum of the N of the output's segments; c = 1 for mask_scale, + 1 for the += (|old| joins the terms);
  * grad-weight: n = the group's rows; c = S - 1 additions of the S slabs, + 1 for the +=; one slab: n = the slice's rows, c = 0;
  * db:          n = the group's rows of |dz|, c as for dW.
The products of bf16 operands are exact in fp32, so CDC_PREC_BF16 has the same bound on the ROUNDED operands (bn_ref.bf16_round
before the float64 contraction).  For the fp32 MFMA the bound is derived (a k-ordered fmaf chain: n roundings of the running
sum).  For the bf16 MFMA it is the starting point the issue sets: any order of fp32 additions of the exact products meets it;
tests/test_gpu_glinear.py records the used fraction.  Measured on an MI355X (profiles/glinear_margins.txt, one clean run of the
whole module): the bf16 launches use at most 0.07 of the bound of y, 0.11 of dx, 0.02 of db, 0.08 of a dW and 0.42 of a single
slab (a 37-row slice; 0.50 where ONE product is added to an old value: a single rounding), so the bf16 MFMA gets NO allowance
beyond the derived c.  Nothing is looser than the suite's present figures: Y_FIG for y, G_FIG for dx, dW and db (helpers.capped).
db: the fp32 kernel and the register-staged bf16 kernel sum the UNROUNDED dz, the shadow kernel the bf16 dz (db_rounded)."""
import numpy as np

from bn_ref import bf16_round, keep_mask_uniform
from helpers import capped, sum_bound

BF16, F32 = 0, 1
Y_FIG = (2e-5, 2e-5)                   # tests/test_gpu_gemm2.py, y
G_FIG = (1e-4, 1e-4)                   # tests/test_gpu_ops.py::test_glinear_fwd_bwd, gradients
SEED = 0x0123_4567_89AB_CDEF
f64 = lambda a: np.asarray(a, dtype=np.float64)
f32 = lambda a: np.asarray(a, dtype=np.float32)

DEFECTS = ("k_tail", "slice_last_row", "slice_twice", "seg_omitted", "mask_extra_col", "no_mask_scale", "acc_off", "no_bias",
           "relu_extra_col", "ragged_off", "db_kind", "operand_unrounded", "slab_db_after_next_dw")


def _op(a, prec, rounded=True):
    return f64(bf16_round(a)) if (prec == BF16 and rounded) else f64(a)


def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def offsets(rows):
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def fwd_case(name, K, Ms, Ns, bias=True, act=None, relu=1, p=0.0, step=None, rows=None, M_arg=None):
    """groups g share one x; Ms[g] rows (dense) or rows[g] rows from offsets(rows)[g] (ragged; M_arg = the M handed over, an
    upper bound).  bias / act: one value or one per group (act None = N)."""
    G = len(Ns)
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * G
    Ms = per(Ms)
    act = [n if a is None else a for a, n in zip(per(act), Ns)]
    return dict(kind="fwd", name=name, K=K, Ms=Ms, Ns=list(Ns), bias=per(bias), act=act, relu=relu, p=p, step=step, rows=rows,
                M_arg=M_arg, R=int(sum(rows)) if rows is not None else max(max(Ms), 1))


def group_rows(c, g, defect=None):
    """(first row, row count) of group / output g"""
    if c["rows"] is None:
        return 0, (c["Ms"][g] if c["kind"] != "bwdx" else c["M"])
    off = offsets(c["rows"])
    lo, hi = int(off[g]), int(off[g + 1])
    if defect == "ragged_off" and hi > lo and lo > 0:
        return lo - 1, hi - lo
    return lo, hi - lo


def keep_scale(p):
    return float(np.float32(1) / (np.float32(1) - np.float32(p))) if p > 0 else 1.0


def fwd_keep(c, g, row_lo, Mg):
    return keep_mask_uniform(SEED, c["step"], g - 64, np.arange(row_lo, row_lo + Mg), c["Ns"][g], c["p"])


def ref_fwd(c, D, prec, defect=None):
    out = {}
    rx = not (defect == "operand_unrounded")
    for g, N in enumerate(c["Ns"]):
        lo, Mg = group_rows(c, g, defect)
        x, w = _op(D["x"][lo:lo + Mg], prec, rx), _op(D["w"][g], prec)
        if defect == "k_tail":
            x, w = x[:, :-1], w[:, :-1]
        y, t = x @ w.T, np.abs(x) @ np.abs(w).T
        n_round = 0
        if c["bias"][g] and defect != "no_bias":
            y, t, n_round = y + f64(D["b"][g]), t + np.abs(f64(D["b"][g])), 1
        a = c["act"][g] + (1 if defect == "relu_extra_col" and c["act"][g] < N else 0)
        bound = sum_bound(t, c["K"], n_round)
        if a > 0 and c["relu"]:
            y[:, :a] = np.maximum(y[:, :a], 0.0)
        if a > 0 and c["p"] > 0:
            keep, ks = fwd_keep(c, g, lo, Mg)[:, :a], keep_scale(c["p"])
            y[:, :a] = np.where(keep, y[:, :a] * ks, 0.0)
            bound[:, :a] = np.where(keep, sum_bound(t[:, :a] * ks, c["K"], n_round + 1), 0.0)
        out[f"y{g}"] = (y, capped(bound, y, Y_FIG))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# grad-input
# ------------------------------------------------------------------------------------------------------------------------
def bwdx_case(name, M, outs, segs, mask_scale=1.0, rows=None, M_arg=None):
    """outs: (K, mask_cols or None for no mask, accumulate) per output; segs: (N, out) per segment, in launch order"""
    return dict(kind="bwdx", name=name, M=M, outs=[tuple(o) for o in outs], segs=[tuple(s) for s in segs], mask_scale=mask_scale,
                rows=rows, M_arg=M_arg, R=int(sum(rows)) if rows is not None else max(M, 1))


def ref_bwdx(c, D, prec, defect=None, round_w=True):
    out = {}
    ms = 1.0 if defect == "no_mask_scale" else float(np.float32(c["mask_scale"]))
    omit = max((s for s, (_, o) in enumerate(c["segs"])), default=None) if defect == "seg_omitted" else None
    for o, (K, mcols, acc) in enumerate(c["outs"]):
        lo, Mo = group_rows(c, o, defect)
        d, t, n = np.zeros((Mo, K)), np.zeros((Mo, K)), 0
        for s, (N, so) in enumerate(c["segs"]):
            if so != o or s == omit:
                continue
            dz, w = _op(D["dz"][s][lo:lo + Mo], prec), _op(D["w"][s], prec, round_w and defect != "operand_unrounded")
            if defect == "k_tail":
                dz, w = dz[:, :-1], w[:-1]
            d, t, n = d + dz @ w, t + np.abs(dz) @ np.abs(w), n + N
        n_round = 0
        if mcols is not None:
            mc = min(K, mcols + (1 if defect == "mask_extra_col" else 0))
            on = f64(D["mask"][o][lo:lo + Mo, :mc]) > 0
            d[:, :mc], t[:, :mc], n_round = np.where(on, d[:, :mc] * ms, 0.0), np.where(on, t[:, :mc] * abs(ms), 0.0), 1
        if acc and defect != "acc_off":
            old = f64(D["dx0"][o][lo:lo + Mo])
            d, t, n_round = d + old, t + np.abs(old), n_round + 1
        out[f"dx{o}"] = (d, capped(sum_bound(t, max(n, 1), n_round), d, G_FIG))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# grad-weight
# ------------------------------------------------------------------------------------------------------------------------
def bwdw_case(name, groups, split=1, defer=0, rows=None, M_arg=None):
    """groups: (M, N, K, db present, accumulate, lddw - K) per group"""
    gs = [tuple(g) + (0,) * (6 - len(g)) for g in groups]
    return dict(kind="bwdw", name=name, groups=gs, Ms=[g[0] for g in gs], split=split, defer=defer, rows=rows, M_arg=M_arg,
                R=int(sum(rows)) if rows is not None else max(max(g[0] for g in gs), 1))


def slices(M, S, unit):
    """the row slices as the kernels cut them: chunk = ceil(M / S) rounded up to `unit` rows (32: k_glinear_bwd_w, 64:
    k_glinear_bwd_w_tr and k_g2_tn), at least one unit; slices past M are empty"""
    S = max(S, 1)
    chunk = max(-(-(-(-M // S)) // unit) * unit, unit)
    return [(min(s * chunk, M), max(min(M - s * chunk, chunk), 0)) for s in range(S)]


def slab_layout(c, defect=None):
    """-> ([(offset of dW_g, offset of db_g)], slab stride): [dW_0 | db_0 | dW_1 | db_1 | ...]"""
    off, at = [], 0
    for (_, N, K, *_r) in c["groups"]:
        off.append([at, at + N * K])
        at += N * K + N
    if defect == "slab_db_after_next_dw" and len(off) >= 2:
        (_, N0, K0, *_r), (_, N1, K1, *_r2) = c["groups"][:2]
        off[1][0] = off[0][0] + N0 * K0                    # [dW_0 | dW_1 | db_0 | db_1 | ...]
        off[0][1] = off[1][0] + N1 * K1
        off[1][1] = off[0][1] + N0
    return [tuple(o) for o in off], at


def ref_bwdw(c, D, prec, unit, db_rounded=False, defect=None):
    """dW / db of every group as the launch leaves them, and slab<s>_dw<g> / slab<s>_db<g> of a split launch"""
    out = {}
    S = max(c["split"], 1)
    if defect == "db_kind":
        db_rounded = not db_rounded
    for g, (M, N, K, has_db, acc, _ld) in enumerate(c["groups"]):
        lo, Mg = group_rows(c, g, defect)
        dz, x = _op(D["dz"][g][lo:lo + Mg], prec), _op(D["x"][g][lo:lo + Mg], prec, defect != "operand_unrounded")
        dzb = f64(bf16_round(D["dz"][g][lo:lo + Mg])) if db_rounded else f64(D["dz"][g][lo:lo + Mg])
        if defect == "k_tail":
            dz, x, dzb = dz[:-1], x[:-1], dzb[:-1]
        dw, tw, db, tb = np.zeros((N, K)), np.zeros((N, K)), np.zeros(N), np.zeros(N)
        sl = slices(len(dz), S, unit)
        first = next((i for i, (_, rn) in enumerate(sl) if rn > 0), None)
        for s, (r0, rn) in enumerate(sl):
            if defect == "slice_last_row" and s == first:
                rn -= 1
            rep = 2 if (defect == "slice_twice" and s == first and S > 1) else 1
            a, b, ab = dz[r0:r0 + rn], x[r0:r0 + rn], dzb[r0:r0 + rn]
            pw, ptw, pb, ptb = a.T @ b * rep, np.abs(a).T @ np.abs(b) * rep, ab.sum(0) * rep, np.abs(ab).sum(0) * rep
            if S > 1:
                out[f"slab{s}_dw{g}"] = (pw, capped(sum_bound(ptw, max(rn, 1), 0), pw, G_FIG))
                if has_db:
                    out[f"slab{s}_db{g}"] = (pb, capped(sum_bound(ptb, max(rn, 1), 0), pb, G_FIG))
            dw, tw, db, tb = dw + pw, tw + ptw, db + pb, tb + ptb
        n_round = S - 1
        if acc and defect != "acc_off":
            dw, tw, db, tb = dw + f64(D["dw0"][g]), tw + np.abs(f64(D["dw0"][g])), db + f64(D["db0"][g]), tb + np.abs(f64(D["db0"][g]))
            n_round += 1
        if not c["defer"]:
            out[f"dw{g}"] = (dw, capped(sum_bound(tw, max(Mg, 1), n_round), dw, G_FIG))
            if has_db:
                out[f"db{g}"] = (db, capped(sum_bound(tb, max(Mg, 1), n_round), db, G_FIG))
    return out


def slab_sums(c, W, wb, defect=None):
    """the slabs [S, stride] (float64 want, bound) of a deferred launch laid out as the header documents; sums over the slices
    give what the consumer adds up"""
    off, stride = slab_layout(c, defect)
    S = c["split"]
    want, bound = np.full((S, stride), np.nan), np.full((S, stride), np.nan)
    for s in range(S):
        for g, (_, N, K, has_db, *_r) in enumerate(c["groups"]):
            want[s, off[g][0]:off[g][0] + N * K], bound[s, off[g][0]:off[g][0] + N * K] = W[f"slab{s}_dw{g}"][0].ravel(), wb[f"slab{s}_dw{g}"][1].ravel()
            if has_db:
                want[s, off[g][1]:off[g][1] + N], bound[s, off[g][1]:off[g][1] + N] = W[f"slab{s}_db{g}"][0], wb[f"slab{s}_db{g}"][1]
    return want, bound


# ------------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------------
def make_data(c):
    rng = _rng(c["name"])
    n = lambda *s, scale=1.0: f32(scale * rng.standard_normal(s))
    R = c["R"]
    if c["kind"] == "fwd":
        K = c["K"]
        return dict(x=n(R, K), w=[n(N, K, scale=K ** -0.5) for N in c["Ns"]], b=[n(N, scale=0.3) for N in c["Ns"]])
    if c["kind"] == "bwdx":
        D = dict(dz=[n(R, N) for N, _ in c["segs"]], w=[n(N, c["outs"][o][0], scale=N ** -0.5) for N, o in c["segs"]],
                 mask=[], dx0=[n(R, K) for K, _, _ in c["outs"]])
        for K, _, _ in c["outs"]:
            m = n(R, K)
            m[rng.random((R, K)) < 0.1] = 0.0              # exact zeros and negative zeros: both mask the gradient
            m[rng.random((R, K)) < 0.1] = -0.0
            D["mask"].append(m)
        return D
    D = dict(dz=[], x=[], dw0=[], db0=[])
    for (_, N, K, *_r) in c["groups"]:
        D["dz"].append(n(R, N)), D["x"].append(n(R, K)), D["dw0"].append(n(N, K)), D["db0"].append(n(N))
    return D


# ------------------------------------------------------------------------------------------------------------------------
# the launches tests/test_gpu_glinear.py runs and tests/test_glinear_ref_cpu.py seeds the defects at
# reduction lengths: 8 tail only, 32 one slab, 40 slab + tail, 64 two slabs (two in flight), 96 three (odd count), 100 three + tail
# ------------------------------------------------------------------------------------------------------------------------
RAGGED4 = (70, 0, 37, 130)                                 # offsets 0, 70, 70, 107, 237: none but 0 a multiple of 64


def fwd_cases():
    return [
        fwd_case("f_tail", 8, 1, [1, 64], bias=[True, False], act=[0, 30]),
        fwd_case("f_one", 32, 63, [3, 65], act=[2, 65], relu=0),
        fwd_case("f_onetail", 40, 64, [64, 129], bias=[False, True], act=[0, 127]),
        fwd_case("f_two", 64, 65, [65, 3], act=[33, 1]),
        fwd_case("f_three", 96, 130, [129, 1], act=[129, 0]),
        fwd_case("f_threetail", 100, [130, 0, 65], [64, 5, 3], bias=[True, True, False], act=[10, 3, 0]),
        fwd_case("f_drop", 40, 130, [65, 64], act=[63, 64], p=0.2, step=None),
        fwd_case("f_dropstep", 64, 65, [129, 3], act=[129, 2], p=0.2, step=77, relu=0),
        fwd_case("f_ragged", 40, None, [65, 3, 64, 129], act=[5, 3, 0, 66], rows=RAGGED4, bias=[True, False, True, True]),
        fwd_case("f_raggeddrop", 96, None, [64, 1, 65, 3], act=[64, 1, 7, 0], rows=RAGGED4, p=0.2, step=5, M_arg=300),
    ]


def bwdx_cases():
    """(case, operand forms it is run in): "w", "wt", "wth" (bf16 transposed copies; every N a multiple of 8), "mix" (some
    segments carry wt: the launch must take the w path)"""
    seg32 = [(8, s % 3) for s in range(32)]
    return [
        (bwdx_case("x_tail", 1, [(1, None, 0)], [(8, 0)]), ("w", "wt", "wth")),
        (bwdx_case("x_one", 63, [(3, 2, 0)], [(32, 0)], mask_scale=1.25), ("w", "wt", "wth")),
        (bwdx_case("x_three", 64, [(64, 61, 1), (65, None, 0)], [(40, 0), (64, 1), (96, 0)], mask_scale=1.25), ("w", "wt", "wth", "mix")),
        (bwdx_case("x_two", 65, [(129, 127, 0)], [(64, 0)], mask_scale=2.0), ("w", "wt", "wth")),
        (bwdx_case("x_odd", 130, [(65, 65, 1)], [(96, 0)], mask_scale=1.25), ("w", "wt", "wth")),
        (bwdx_case("x_fallback", 130, [(64, 3, 0), (3, None, 1)], [(100, 0), (100, 1)], mask_scale=1.25), ("w", "wt")),
        (bwdx_case("x_unaligned_n", 65, [(64, None, 0)], [(3, 0), (65, 0)]), ("w", "wt")),
        (bwdx_case("x_seg32", 65, [(3, 2, 0), (64, None, 1), (1, None, 0)], seg32, mask_scale=1.25), ("w", "wt", "wth")),
        (bwdx_case("x_unnamed", 63, [(64, 5, 0), (3, None, 0), (65, 2, 1)], [(64, 0), (32, 0)], mask_scale=1.25), ("w", "wt", "wth", "mix")),
        (bwdx_case("x_ragged", None, [(64, 61, 0), (65, None, 1), (3, None, 0), (129, 7, 1)], [(64, 0), (40, 1), (96, 3), (8, 2), (32, 3)],
                   mask_scale=1.25, rows=RAGGED4), ("w", "wt", "wth")),
    ]


def bwdw_cases(form):
    """form: "f32" (k_glinear_bwd_w), "tr" (k_glinear_bwd_w_tr), "sh" (shadows: k_g2_tn, both tile classes)"""
    S = [
        bwdw_case(f"w_{form}_1", [(1, 1, 8, 1, 0, 0), (1, 64, 3, 0, 1, 0)]),
        bwdw_case(f"w_{form}_31", [(31, 3, 65, 1, 1, 2), (31, 64, 64, 1, 0, 0)], split=2),
        bwdw_case(f"w_{form}_64", [(64, 64, 40, 1, 0, 0), (64, 5, 129, 0, 0, 3)], split=3),
        bwdw_case(f"w_{form}_65", [(65, 63, 64, 1, 0, 0), (65, 3, 1, 1, 0, 0)], split=8),
        bwdw_case(f"w_{form}_200", [(200, 64, 96, 1, 1, 0), (200, 1, 100, 1, 0, 5)], split=5),
        bwdw_case(f"w_{form}_1000", [(1000, 33, 65, 1, 0, 0), (1000, 64, 8, 0, 0, 0)], split=8),
        bwdw_case(f"w_{form}_1000one", [(1000, 3, 32, 1, 1, 0)]),
        bwdw_case(f"w_{form}_defer", [(200, 64, 40, 1, 0, 0), (200, 3, 65, 1, 0, 1), (65, 5, 8, 0, 0, 0)], split=3, defer=1),
        bwdw_case(f"w_{form}_defer65", [(65, 8, 12, 1, 0, 0), (65, 4, 8, 1, 0, 0)], split=8, defer=1),
    ]
    if form == "sh":
        S += [bwdw_case("w_sh_wide", [(200, 129, 65, 1, 0, 0), (200, 64, 130, 1, 1, 2)], split=2),
              bwdw_case("w_sh_wide1", [(65, 65, 64, 1, 0, 0)]),
              bwdw_case("w_sh_widedefer", [(1000, 130, 96, 1, 0, 0), (1000, 3, 129, 0, 0, 0)], split=5, defer=1)]
    else:
        S += [bwdw_case(f"w_{form}_ragged", [(None, 65, 40, 1, 0, 0), (None, 3, 64, 1, 1, 0), (None, 64, 3, 0, 0, 2), (None, 5, 129, 1, 0, 0)],
                        split=2, rows=RAGGED4),
              bwdw_case(f"w_{form}_ragged1", [(None, 64, 64, 1, 1, 0), (None, 3, 8, 1, 0, 0), (None, 1, 1, 1, 0, 0), (None, 65, 100, 0, 0, 0)],
                        rows=RAGGED4, M_arg=300)]
    return S


def all_ref_runs():
    """every (tag, case, precision, kwargs of the ref function) the GPU module compares a launch with"""
    runs = []
    for c in fwd_cases():
        runs += [("fwd", c, prec, {}) for prec in (BF16, F32)]
    for c, _forms in bwdx_cases():
        runs += [("bwdx", c, prec, {}) for prec in (BF16, F32)]
    for form, prec, unit, rounded in (("f32", F32, 32, False), ("tr", BF16, 64, False), ("sh", BF16, 64, True)):
        runs += [("bwdw", c, prec, dict(unit=unit, db_rounded=rounded)) for c in bwdw_cases(form)]
    return runs


def ref(tag, c, D, prec, defect=None, **kw):
    return {"fwd": ref_fwd, "bwdx": ref_bwdx, "bwdw": ref_bwdw}[tag](c, D, prec, defect=defect, **kw)
