"""float64 restatement of what include/cdcmdr.h promises for the PLE level boundary (cdc_cgc_mid_fwd / _bwd, csrc/cgc.hip) and for
the narrow gate pooling (cdc_gate_pool_fwd / _bwd, csrc/rowops.hip), every value with a DERIVED error bound, an fp32 / bf16
restatement in the kernels' operation order that stands in for a device on the CPU, the case lists tests/test_gpu_cgc_direct.py
runs, and the seeded defects the bounds have to reject.  No GPU: tests/test_cgc_ref_cpu.py holds this file,
tests/test_gpu_cgc_direct.py holds the launches to it.

The chain is discontinuous (the bf16 roundings of the pooled vectors, of dZ and of the gate-logit gradients; ReLU; dropout), so the
reference is STAGE-WISE: every stage is computed in float64 from what the launch itself saved for the stage before (`S`), so that
one bf16 rounding flip does not have to be absorbed by every later bound.  With S = None the stages are chained on their own
float64 results (nothing rounded): that composition is what tests/test_cgc_ref_cpu.py holds against torch autograd.

Forward stages (ref_mid_fwd; counts are written (n_exp1, n_gate1, n_exp2, n_gate2), widths (H1, H2) = (128, 64)):
  probs1_g   = softmax(logits1_g)
  pooled_h_g = bf16( sum_j probs1_g[j] ex1[:, sel1_g[j]] ), terms in list order                      (from the launch's probs1)
  ex2        = drop(relu(pooled_h[src_e] W_e^T + bias_e)) per expert e                                (from the launch's pooled_h)
  probs2_t   = softmax(pooled_h[src_t] Wg_t^T + bg_t)                                                 (from the launch's pooled_h)
  out_t      = sum_j probs2_t[j] ex2[:, sel2_t[j]];  outh_t = bf16(out_t)                             (from the launch's probs2, ex2)
Backward stages (ref_mid_bwd; inputs ex1, ex2, probs1, probs2 = the chained reference forward rounded to fp32, d_out random):
  dz2_h      = bf16( mask2( sum over the gates t selecting e, in gate order, of probs2_t[pos] d_out_t ) )
  dl2_t[j]   = p_j (dp_j - sum_k p_k dp_k),  dp_j = <d_out_t, ex2[sel2_t[j]]> over 64 terms
  dP1_s      = sum_{e: src = s} dz2_h[e] W_e + sum_{t: src = s} bf16(dl2_t) Wg_t   (fp32, at most 6 K steps of 32; NOT an output:
               its bound joins the next two stages;                                  from the launch's dz2_h and dl2)
  dz1_h      = bf16( mask1( sum_g probs1_g[pos] dP1_g ) )
  dl1_g[j]   from dp1_j = <dP1_g, ex1[sel1_g[j]]> over 128 terms
The same pooling stages serve cdc_gate_pool_fwd / _bwd (ref_pool_fwd / ref_pool_bwd): there out, d_experts and d_logits are fp32,
accumulate = 1 adds to a pre-fill, mask_relu / mask_scale as in the header.

Every ref_* function returns name -> (want, bound).  compare() holds
  * an fp32 output to |got - want| <= bound (helpers.assert_bounded);
  * a bf16 output that has no fp32 twin (pooled_h, dz1_h, dz2_h, out_h when out is NULL) to "got is the bf16 rounding of SOME value
    within the bound of want": bf16(want - b) <= got <= bf16(want + b), rounding to nearest even being monotonic.  It is not a bare
    relative tolerance: with b = 0 it is bit equality;
  * a bf16 shadow written beside its fp32 twin (out_h, d_logits_h, d_experts_h) to the bits of bf16(the fp32 value the launch wrote).

The bounds, from the kernels' arithmetic (the library is built with -ffp-contract=off; helpers.sum_bound(terms, n, c) =
(n + c) 2^-24 sum |term|):
  * softmax over n <= 16 inputs, as the kernels form it (max, v - max, expf, sum in index order, one reciprocal, one product).  With
    d_j = max - l_j the argument's rounding is at most 2^-24 d_j, which exp turns into a RELATIVE error of 2^-24 d_j; expf itself is
    allowed EXPF_ULPS = 2 ulps (HIP documents 1 for expf), i.e. 4 x 2^-24: e_j = (d_j + 4) 2^-24.  The sum of n positive terms adds
    n roundings and carries the p-weighted mean of the e_k, the reciprocal and the product one rounding each:
        |dp_j| <= p_j (e_j + sum_k p_k e_k + (n + 2) 2^-24) + 2^-126
    (2^-126: a probability below the smallest normal number may be flushed to zero).
  * softmax of COMPUTED logits (probs2: the logits are no output).  If every logit of a row is within delta of its float64 value,
    softmax being shift-invariant, p'_j = e^{l_j + a_j} / sum_k e^{l_k + a_k} with |a| <= delta lies in [p_j e^{-2 delta},
    p_j e^{2 delta}], so |p'_j - p_j| <= p_j (e^{2 delta} - 1); the softmax's own terms above then act on p' <= p_j e^{2 delta}:
        |dp_j| <= p_j (e^{2 delta} - 1) + e^{2 delta} (own bound),   delta = max_j sum_bound(sum |a w| + |bg|, 128, 1)_j.
  * pooling: products of two fp32 values, added in list order: one rounding per product and at most n - 1 per partial sum:
    sum_bound(sum |p x|, n_sel, 0).
  * the bf16 MFMA contractions (ex2, gate logits, dP1): products of bf16 operands are exact in fp32, so n = K roundings at most
    whatever the order, + 1 for the bias, + 1 for the product with the dropout scale; the scale is the fp32 value the kernel forms,
    1 / (1 - p) in fp32.  A dropped element and an expert no gate selects are EXACTLY 0: bound 0.
  * expert gradients: sum_bound(sum |p d|, gates selecting e, 1 with the mask's scale); where the summands are dP1 (level k) each
    carries dP1's own bound sum_bound(sum |dz w| + sum |dl wg|, 32 x K steps, 0), weighted by p.
  * gate-logit gradients: dp_j over H terms: sum_bound(sum |d x|, H, 0) (+ sum |x| x dP1's bound at level k) = b_j;
    dot = sum_k p_k dp_k: sum_k p_k b_k + sum_bound(sum |p dp|, n, 0) = b_dot; one subtraction and one product:
        |d dl_j| <= p_j (b_j + b_dot) + 2 x 2^-24 p_j (|dp_j| + |dot|).
  * accumulate = 1 (pool backward): one more addition, the pre-fill among the terms.
  * a product with a probability below the smallest normal number may lose bits or be flushed to zero: 2^-126 per such term
    (pooling, expert gradients: one per selected term; gate-logit gradients: n_sel + 2).
Every bound is capped (helpers.capped) by OUT_FIG, or by SUM_FIG where the value is or carries a dot product over a row (ex2, the
gate-logit gradients, dz1_h through dP1).  No other figure is used, and no element of any output is excluded.

Which case reaches what is listed in the docstring of tests/test_gpu_cgc_direct.py."""
import numpy as np

import bn_ref as B
from helpers import OUT_FIG, SUM_FIG, U24, assert_bits_equal, assert_bounded, capped, sum_bound

H1, H2 = 128, 64
MID_MAX_EXPERT, MID_MAX_GATE, MAX_SEL, MAX_GATES, MID_MAXSTEP = 16, 8, 16, 16, 6
SEED, STEP = 0x1234_5678_9ABC_DEF1, 5
ROWS_MAX = 67                                    # every case has at most 67 rows; a case's data are the first B rows of 67
TINY = 2.0 ** -126
EXPF_ULPS = 2.0
f64 = lambda a: np.asarray(a, dtype=np.float64)
f32 = lambda a: np.asarray(a, dtype=np.float32)

FWD_DEFECTS = ("softmax_no_max", "wrong_source", "no_bias", "drop_pair_swapped")
BWD_DEFECTS = ("pos_off_by_one", "mask_ge", "no_scale", "dlogits_no_dot", "first_gate_only", "acc_ignored", "last_kstep_dropped",
               "dl_unrounded")
DEFECTS = FWD_DEFECTS + BWD_DEFECTS


# ------------------------------------------------------------------------------------------------------------------------
# the fused boundary: layouts and cases
# ------------------------------------------------------------------------------------------------------------------------
def topology(counts, kind):
    """-> sel1 (per level-k gate), src_e / src_g (the level-k output each level-k+1 expert / gate reads), sel2"""
    ne1, ng1, ne2, ng2 = counts
    if kind in ("ple", "sparse"):                # n towers: two experts per tower + two shared, a gate per tower (+ the shared one)
        T = ng2
        assert (ne1, ng1, ne2) == (2 * T + 2, T + 1, 2 * T + 2)
        own = lambda i: [2 * i, 2 * i + 1, 2 * T, 2 * T + 1]
        src_e, src_g = [e // 2 for e in range(2 * T)] + [T, T], list(range(T))
        if kind == "ple":
            sel1, sel2 = [own(i) for i in range(T)] + [list(range(ne1))], [own(i) for i in range(T)]
        else:                                    # non-prefix lists: experts 1, 3, 7 in every list, experts 0, 5, 6 in none
            lst = lambda g: sorted({1, 3, 7, 2 + 2 * (g % 2)})
            sel1, sel2 = [lst(g) for g in range(ng1)], [lst(t) for t in range(ng2)]
    elif kind == "one":
        assert counts == (1, 1, 1, 1)
        sel1, src_e, src_g, sel2 = [[0]], [0], [0], [[0]]
    elif kind == "steps":                        # source 0: three experts (6 K steps), 1: two experts + two gates (6), 2: one gate (1)
        assert counts == (4, 3, 5, 3)
        sel1, src_e, src_g, sel2 = [[0, 1, 2, 3], [1, 3], [2]], [0, 0, 0, 1, 1], [1, 1, 2], [[0, 1, 2, 3, 4], [1, 3], [0, 2, 4]]
    elif kind == "max":                          # both maxima; K steps per source 6, 6, 1, 6, 6, 5, 5, 5; a gate with n_sel = 16
        assert counts == (4, 8, 16, 8)
        src_e, src_g = [0, 0, 0, 1, 1, 3, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7], [1, 1, 2, 4, 4, 5, 6, 7]
        sel1 = [[0, 1, 2, 3] if g % 2 == 0 else [1, 3] for g in range(8)]
        sel1[2] = [2]
        sel2 = [list(range(16)), [1, 3, 7]] + [[1, 3, 7, 8 + t] for t in range(2, 8)]
    else:
        raise ValueError(kind)
    assert len(sel1) == ng1 and len(src_e) == ne2 and len(src_g) == ng2 and len(sel2) == ng2
    return dict(sel1=sel1, src_e=src_e, src_g=src_g, sel2=sel2)


def k_steps(c, s, defect=None):
    """the K steps of source s's grad-input tile: ("e", expert, half) for the experts reading it (ascending), then ("g", gate)"""
    T = c["topo"]
    steps = [("e", e, h) for e in range(c["counts"][2]) if T["src_e"][e] == s for h in (0, 1)]
    steps += [("g", t, 0) for t in range(c["counts"][3]) if T["src_g"][t] == s]
    if defect == "last_kstep_dropped" and len(steps) == MID_MAXSTEP:
        steps = steps[:-1]
    return steps


def mid(name, counts=(8, 4, 8, 3), kind="ple", B=17, p=0.2, step=STEP, relu=1, bias=True, null=(), mask1=1, mask2=1, scales=None,
        dlh=False, data=None):
    """step: the value behind seed_offset_dev, None = NULL.  null: of "pooled_h", "out", "out_h" (in every gate).  scales: (scale1,
    scale2) of the backward's masks, None = the dropout scale.  dlh: d_logits_h of both levels present.  data: the case whose data
    this one shares (its first B rows)."""
    assert set(null) <= {"pooled_h", "out", "out_h"} and not {"out", "out_h"} <= set(null) and B <= ROWS_MAX
    c = dict(op="mid", name=name, counts=tuple(counts), kind=kind, B=B, p=p, step=step, relu=relu, bias=bias, null=tuple(null),
             mask1=mask1, mask2=mask2, dlh=dlh, data=data or name, topo=topology(tuple(counts), kind))
    ks = float(keep_scale(p))
    c["scales"] = tuple(scales) if scales else (ks, ks)
    c["stream_id"] = [64 + 3 + e for e in range(counts[2])]          # distinct per expert
    for s in range(counts[1]):
        assert 1 <= len(k_steps(c, s)) <= MID_MAXSTEP
    return c


def mid_cases():
    S = [mid(f"ple3_b{b}", B=b, data="ple3", dlh=b == 35) for b in (1, 15, 16, 17, 35)]
    S += [mid("tower5_b17", (12, 6, 12, 5), B=17, data="tower5", dlh=True), mid("tower5_b35", (12, 6, 12, 5), B=35, data="tower5"),
          mid("one_b1", (1, 1, 1, 1), "one", B=1, data="one"), mid("one_b17", (1, 1, 1, 1), "one", B=17, data="one"),
          mid("max_b16", (4, 8, 16, 8), "max", B=16, data="max"), mid("max_b17", (4, 8, 16, 8), "max", B=17, data="max", dlh=True),
          mid("steps_b17", (4, 3, 5, 3), "steps"), mid("steps_b35", (4, 3, 5, 3), "steps", B=35, p=0.5),
          mid("sparse_b17", kind="sparse"),
          mid("p0", p=0.0, data="ple3"), mid("p05", p=0.5, data="ple3"), mid("nostep", step=None, data="ple3"),
          mid("relu0", relu=0, p=0.0, mask2=0, data="ple3"), mid("nobias", bias=False, data="ple3"),
          mid("mask1off", mask1=0, data="ple3"), mid("mask2off", mask2=0, data="ple3"), mid("scales", scales=(1.25, 3.0), data="ple3")]
    S += [mid(f"null_{k}", null=(k,), data="ple3") for k in ("pooled_h", "out", "out_h")]
    assert len({c["name"] for c in S}) == len(S)
    return S


def pool(name, H=64, B=5, n_expert=4, sels=None, acc=0, mask=1, scale=1.25, unaligned=False, data=None):
    """sels: one selection list per gate (list order = summation order; not necessarily ascending).  unaligned: an odd ld_exp
    (forces the scalar kernels)."""
    sels = [list(s) for s in (sels or [[0, 1], [1, 3], [3, 1, 0]])]         # experts 1, 3 shared, expert 2 unselected, one descending
    assert all(0 < len(s) <= MAX_SEL and max(s) < n_expert for s in sels) and len(sels) <= MAX_GATES and n_expert <= 2 * MAX_SEL
    return dict(op="pool", name=name, H=H, B=B, n_expert=n_expert, sels=sels, acc=acc, mask=mask, scale=scale, unaligned=unaligned,
                data=data or name)


def pool_cases():
    S = [pool(f"h{H}", H=H) for H in (4, 12, 64, 128, 256, 320)]
    S += [pool("h64_unaligned", unaligned=True, data="h64"),
          pool("e16", n_expert=16, sels=[list(range(16)), [15, 0, 7], [7]]),
          pool("e17", n_expert=17, sels=[list(range(1, 17)), [16, 0], [16]]),
          pool("e32", n_expert=32, sels=[list(range(0, 32, 2)), [31, 1, 30], [31]]),
          pool("g1", sels=[[2]]), pool("g16", n_expert=6, sels=[[g % 6, (g + 1 + g // 6) % 6] for g in range(15)] + [list(range(6))]),
          pool("acc1", acc=1), pool("acc1_h12", H=12, acc=1), pool("mask0", mask=0), pool("mask0_h320", H=320, mask=0, acc=1),
          pool("b1", B=1), pool("b67", B=67), pool("b67_h128", H=128, B=67), pool("b67_h12", H=12, B=67)]
    assert len({c["name"] for c in S}) == len(S)
    return S


def by_name(name):
    return next(c for c in mid_cases() + pool_cases() if c["name"] == name)


def keep_scale(p):
    """1 / (1 - p) as the kernel forms it: in fp32"""
    return np.float32(1) / (np.float32(1) - np.float32(p)) if p > 0 else np.float32(1)


def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def _logits(rng, n_sel, g):
    """one row at 1e4, one of equal logits, one spread over +-80 (rows g, g + 1, g + 2 modulo 5: row 0 of gate 0 is the 1e4 row)"""
    l = f32(rng.standard_normal((ROWS_MAX, n_sel)))
    l[g % 5] += np.float32(1e4)
    l[(g + 1) % 5] = np.float32(0.5)
    l[(g + 2) % 5] = np.linspace(-80.0, 80.0, n_sel, dtype=np.float32) if n_sel > 1 else np.float32(80.0)
    return l


def _activations(rng, cols):
    """what a relu + dropout layer writes: about 60 % exact zeros, so that a `>= 0` mask shows"""
    x = f32(np.maximum(rng.standard_normal((ROWS_MAX, cols)), 0.0))
    x[rng.random((ROWS_MAX, cols)) < 0.2] = 0.0
    return x


def make_data(c):
    """seeded by c["data"]; weights hold bf16-representable values (the test writes their bits).  ROWS_MAX rows are drawn, the case
    takes the first B: cases that share data share rows."""
    rng = _rng(c["op"] + c["data"])
    n = c["B"]
    if c["op"] == "pool":
        D = dict(ex=_activations(rng, c["n_expert"] * c["H"])[:n], logits=[_logits(rng, len(s), g)[:n] for g, s in enumerate(c["sels"])],
                 dout=[f32(rng.standard_normal((ROWS_MAX, c["H"])))[:n] for _ in c["sels"]],
                 dex0=f32(rng.standard_normal((ROWS_MAX, c["n_expert"] * c["H"])))[:n])
        return D
    ne1, ng1, ne2, ng2 = c["counts"]
    T = c["topo"]
    D = dict(ex1=_activations(rng, ne1 * H1)[:n], logits1=[_logits(rng, len(T["sel1"][g]), g)[:n] for g in range(ng1)])
    D["W"] = [B.bf16_round(f32(rng.standard_normal((H2, H1)) / np.sqrt(H1))) for _ in range(ne2)]
    D["b"] = [f32(0.3 * rng.standard_normal(H2)) for _ in range(ne2)]
    D["Wg"] = [B.bf16_round(f32(rng.standard_normal((len(T["sel2"][t]), H1)) / np.sqrt(H1))) for t in range(ng2)]
    D["bg"] = [f32(0.3 * rng.standard_normal(len(T["sel2"][t]))) for t in range(ng2)]
    D["dout"] = [f32(rng.standard_normal((ROWS_MAX, H2)))[:n] for _ in range(ng2)]
    return D


# ------------------------------------------------------------------------------------------------------------------------
# the stages, float64
# ------------------------------------------------------------------------------------------------------------------------
def softmax_ref(l, dl=None, defect=None):
    """l [B, n] logits; dl: the bound of computed logits (None: inputs, exact) -> (p, bound)"""
    l = f64(l)
    n = l.shape[1]
    m = l.max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(l) if defect == "softmax_no_max" else np.exp(l - m)
        p = e / e.sum(1, keepdims=True)
    ej = ((m - l) + 2 * EXPF_ULPS) * U24
    b = p * (ej + (p * ej).sum(1, keepdims=True) + (n + 2) * U24) + TINY
    if dl is not None:
        g = np.exp(2 * f64(dl).max(1, keepdims=True))
        b = p * (g - 1) + g * b
    return p, capped(b, p, OUT_FIG)


def _experts(x, H):
    x = f64(x)
    return x.reshape(x.shape[0], -1, H)


def pool_ref(p, x, sel, H):
    """sum_j p[:, j] x[:, sel[j]] -> (want [B, H], sum |terms|)"""
    X = _experts(x, H)[:, sel, :]
    p = f64(p)[:, :, None]
    return (p * X).sum(1), (np.abs(p) * np.abs(X)).sum(1)


def pool_out(p, x, sel, H):
    w, mag = pool_ref(p, x, sel, H)
    return w, capped(sum_bound(mag, len(sel), 0) + len(sel) * TINY, w, OUT_FIG)


def linear_ref(a, W, b):
    a, W = f64(a), f64(W)
    z, mag = a @ W.T, np.abs(a) @ np.abs(W).T
    if b is not None:
        z, mag = z + f64(b), mag + np.abs(f64(b))
    return z, mag


def expert_grad_ref(P, DO, sels, n_expert, H, x, mask, scale, fig, dDO=None, defect=None, old=None):
    """d_expert_e = mask( sum over the gates g selecting e, in gate order, of P[g][:, pos] DO[g] ) (+ old) -> ([B, n_expert H], bound).
    dDO: the bounds of the DO themselves."""
    n = f64(DO[0]).shape[0]
    want, mag, carried, cnt = np.zeros((n, n_expert, H)), np.zeros((n, n_expert, H)), np.zeros((n, n_expert, H)), np.zeros(n_expert)
    for e in range(n_expert):
        for g, sel in enumerate(sels):
            if e not in sel:
                continue
            j = sel.index(e)
            if defect == "pos_off_by_one":
                j = (j + 1) % len(sel)
            pj = f64(P[g])[:, j:j + 1]
            want[:, e] += pj * f64(DO[g])
            mag[:, e] += np.abs(pj * f64(DO[g]))
            if dDO is not None:
                carried[:, e] += np.abs(pj) * dDO[g]
            cnt[e] += 1
            if defect == "first_gate_only":
                break
    bound = sum_bound(mag, cnt[None, :, None], 1 if mask else 0) + carried + cnt[None, :, None] * TINY
    if mask:
        X = _experts(x, H)
        on = X >= 0 if defect == "mask_ge" else X > 0
        s = 1.0 if defect == "no_scale" else float(scale)
        want, bound = np.where(on, want * s, 0.0), np.where(on, bound * abs(s), 0.0)
    want, bound = want.reshape(n, -1), bound.reshape(n, -1)
    if old is not None and defect != "acc_ignored":
        want = f64(old) + want
        bound = bound + U24 * np.abs(want)
    return want, capped(bound, want, fig)


def dlogits_ref(p, DO, x, sel, H, dDO=None, defect=None):
    """p_j (dp_j - sum_k p_k dp_k), dp_j = <DO, x[:, sel[j]]> -> ([B, n_sel], bound)"""
    p, DO = f64(p), f64(DO)
    X = _experts(x, H)[:, sel, :]
    dp, mdp = np.einsum("bh,bjh->bj", DO, X), np.einsum("bh,bjh->bj", np.abs(DO), np.abs(X))
    bdp = sum_bound(mdp, H, 0)
    if dDO is not None:
        bdp = bdp + np.einsum("bh,bjh->bj", dDO, np.abs(X))
    dot = (p * dp).sum(1, keepdims=True)
    bdot = (p * bdp).sum(1, keepdims=True) + sum_bound(np.abs(p * dp).sum(1, keepdims=True), len(sel), 0)
    want = p * dp if defect == "dlogits_no_dot" else p * (dp - dot)
    return want, capped(p * (bdp + bdot) + sum_bound(p * (np.abs(dp) + np.abs(dot)), 0, 2) + (len(sel) + 2) * TINY, want, SUM_FIG)


def drop_keep(c, e, defect=None):
    """keep mask [B, H2] of level-k+1 expert e: the 32-bit counter stream cdc_gemm_bf16_nt draws from, by GLOBAL row"""
    if c["p"] <= 0:
        return np.ones((c["B"], H2), dtype=bool)
    keep = B.keep_mask_bits16(SEED, c["step"], c["stream_id"][e] - 64, np.arange(c["B"]), H2, c["p"])
    return keep[:, np.arange(H2) ^ 1] if defect == "drop_pair_swapped" else keep


# ------------------------------------------------------------------------------------------------------------------------
# the fused boundary
# ------------------------------------------------------------------------------------------------------------------------
def ref_mid_fwd(c, D, S=None, defect=None):
    """S: what the launch saved — probs1, pooled_h, probs2 (lists per gate), ex2 [B, n_exp2 H2]; None chains the stages on their own
    float64 results.  R["chained"] holds those."""
    ne1, ng1, ne2, ng2 = c["counts"]
    T, n = c["topo"], c["B"]
    R, W = {}, dict(probs1=[], pooled_h=[], probs2=[])
    for g in range(ng1):
        R[f"probs1_{g}"] = softmax_ref(D["logits1"][g], defect=defect)
        W["probs1"].append(R[f"probs1_{g}"][0])
    src = W if S is None else S
    for g in range(ng1):
        R[f"pooled_h_{g}"] = pool_out(src["probs1"][g], D["ex1"], T["sel1"][g], H1)
        W["pooled_h"].append(R[f"pooled_h_{g}"][0])
    wrong = (lambda s: (s + 1) % ng1) if defect == "wrong_source" else (lambda s: s)
    ks = float(keep_scale(c["p"]))
    ex2, bex2 = np.zeros((n, ne2, H2)), np.zeros((n, ne2, H2))
    for e in range(ne2):
        z, mag = linear_ref(src["pooled_h"][wrong(T["src_e"][e])], D["W"][e], D["b"][e] if (c["bias"] and defect != "no_bias") else None)
        b = sum_bound(mag, H1, 1 + int(c["p"] > 0))
        if c["relu"]:
            z = np.maximum(z, 0.0)
        keep = drop_keep(c, e, defect)
        ex2[:, e], bex2[:, e] = np.where(keep, z * ks, 0.0), np.where(keep, b * ks, 0.0)
    ex2, bex2 = ex2.reshape(n, -1), bex2.reshape(n, -1)
    R["ex2"] = (ex2, capped(bex2, ex2, SUM_FIG))
    W["ex2"] = ex2
    for t in range(ng2):
        z, mag = linear_ref(src["pooled_h"][wrong(T["src_g"][t])], D["Wg"][t], D["bg"][t] if (c["bias"] and defect != "no_bias") else None)
        R[f"probs2_{t}"] = softmax_ref(z, sum_bound(mag, H1, 1), defect)
        W["probs2"].append(R[f"probs2_{t}"][0])
    src = W if S is None else S
    for t in range(ng2):
        R[f"out_{t}"] = pool_out(src["probs2"][t], src["ex2"], T["sel2"][t], H2)
    if "pooled_h" in c["null"]:
        for g in range(ng1):
            del R[f"pooled_h_{g}"]
    R["chained"] = W
    return R


def bwd_inputs(c, D):
    """ex2, probs1, probs2 of the reference forward as fp32 (ex1 and d_out are data): what the backward launch is given"""
    W = ref_mid_fwd(c, D)["chained"]
    return dict(ex2=f32(W["ex2"]), probs1=[f32(v) for v in W["probs1"]], probs2=[f32(v) for v in W["probs2"]])


def ref_mid_bwd(c, D, I, S=None, defect=None):
    """I: bwd_inputs (or the chained float64 forward).  S: the launch's dz2_h [B, n_exp2 H2] and dl2 (list per gate); None chains."""
    ne1, ng1, ne2, ng2 = c["counts"]
    T, n = c["topo"], c["B"]
    R = {}
    R["dz2_h"] = expert_grad_ref(I["probs2"], D["dout"], T["sel2"], ne2, H2, I["ex2"], c["mask2"], c["scales"][1], OUT_FIG, defect=defect)
    for t in range(ng2):
        R[f"dl2_{t}"] = dlogits_ref(I["probs2"][t], D["dout"][t], I["ex2"], T["sel2"][t], H2, defect=defect)
    if S is None:
        dz, dl = R["dz2_h"][0], [R[f"dl2_{t}"][0] for t in range(ng2)]
    else:
        dz = f64(S["dz2_h"])
        dl = [f64(v) if defect == "dl_unrounded" else f64(B.bf16_round(f32(v))) for v in S["dl2"]]
    dz = dz.reshape(n, ne2, H2)
    dP, bP = [], []
    for s in range(ng1):
        v, mag = np.zeros((n, H1)), np.zeros((n, H1))
        steps = k_steps(c, s, defect)
        for kind, i, h in steps:
            a, w = (dz[:, i, 32 * h:32 * h + 32], f64(D["W"][i])[32 * h:32 * h + 32]) if kind == "e" else (dl[i], f64(D["Wg"][i]))
            v, mag = v + a @ w, mag + np.abs(a) @ np.abs(w)
        dP.append(v)
        bP.append(sum_bound(mag, 32 * len(steps), 0))
    R["dz1_h"] = expert_grad_ref(I["probs1"], dP, T["sel1"], ne1, H1, D["ex1"], c["mask1"], c["scales"][0], SUM_FIG, dDO=bP, defect=defect)
    for g in range(ng1):
        R[f"dl1_{g}"] = dlogits_ref(I["probs1"][g], dP[g], D["ex1"], T["sel1"][g], H1, dDO=bP[g], defect=defect)
    R["chained"] = dict(dP1=dP)
    return R


# ------------------------------------------------------------------------------------------------------------------------
# the narrow pool
# ------------------------------------------------------------------------------------------------------------------------
def ref_pool_fwd(c, D, S=None, defect=None):
    R, W = {}, dict(probs=[])
    for g, sel in enumerate(c["sels"]):
        R[f"probs_{g}"] = softmax_ref(D["logits"][g], defect=defect)
        W["probs"].append(R[f"probs_{g}"][0])
    src = W if S is None else S
    for g, sel in enumerate(c["sels"]):
        R[f"out_{g}"] = pool_out(src["probs"][g], D["ex"], sel, c["H"])
    R["chained"] = W
    return R


def pool_bwd_inputs(c, D):
    return dict(probs=[f32(v) for v in ref_pool_fwd(c, D)["chained"]["probs"]])


def ref_pool_bwd(c, D, I, defect=None):
    R = {}
    for g, sel in enumerate(c["sels"]):
        R[f"dl_{g}"] = dlogits_ref(I["probs"][g], D["dout"][g], D["ex"], sel, c["H"], defect=defect)
    R["dex"] = expert_grad_ref(I["probs"], D["dout"], c["sels"], c["n_expert"], c["H"], D["ex"], c["mask"], np.float32(c["scale"]), OUT_FIG,
                               defect=defect, old=D["dex0"] if c["acc"] else None)
    return R


def applies(defect, c):
    if c["op"] == "pool":
        multi = any(sum(e in s for s in c["sels"]) > 1 for e in range(c["n_expert"]))
        return {"softmax_no_max": True, "pos_off_by_one": any(len(s) > 1 for s in c["sels"]), "mask_ge": bool(c["mask"]),
                "no_scale": bool(c["mask"]), "dlogits_no_dot": any(len(s) > 1 for s in c["sels"]), "first_gate_only": multi,
                "acc_ignored": bool(c["acc"])}.get(defect, False)
    T, (ne1, ng1, ne2, ng2) = c["topo"], c["counts"]
    lists = T["sel1"] + T["sel2"]
    multi = any(sum(e in s for s in T["sel2"]) > 1 for e in range(ne2)) or any(sum(e in s for s in T["sel1"]) > 1 for e in range(ne1))
    return {"softmax_no_max": True, "wrong_source": ng1 > 1, "no_bias": c["bias"], "drop_pair_swapped": c["p"] > 0,
            "pos_off_by_one": any(len(s) > 1 for s in lists), "mask_ge": bool(c["mask1"] or c["mask2"]),
            "no_scale": (c["mask1"] and c["scales"][0] != 1) or (c["mask2"] and c["scales"][1] != 1),
            "dlogits_no_dot": any(len(s) > 1 for s in lists), "first_gate_only": multi, "acc_ignored": False,
            "last_kstep_dropped": any(len(k_steps(c, s)) == MID_MAXSTEP for s in range(ng1)), "dl_unrounded": any(len(s) > 1 for s in T["sel2"])}[defect]


# ------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------
BF16_ONLY = ("pooled_h_", "dz1_h", "dz2_h")                      # bf16 outputs without an fp32 twin
SHADOWS = (("out_", "outh_"), ("dl1_", "dl1h_"), ("dl2_", "dl2h_"), ("dl_", "dlh_"), ("dex", "dexh"))


def shadow_of(k):
    for a, b in SHADOWS:
        if k.startswith(a):
            return b + k[len(a):]
    return None


def bf16_round64(v):
    """a float64 value rounded to bf16 (nearest even) in ONE step"""
    v = f64(v)
    _, e = np.frexp(v)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.rint(v / q) * q


def assert_bf16_of_bounded(got, want, bound, what=""):
    """got is the bf16 rounding of some value within `bound` of want: bf16(want - b) <= got <= bf16(want + b), every element"""
    import os
    g, w = f64(got), f64(want)
    b = np.broadcast_to(f64(bound), w.shape)
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    if not g.size:
        return
    lo, hi = bf16_round64(w - b), bf16_round64(w + b)
    rec = os.environ.get("CDC_RECORD_MARGINS")
    if rec:
        # the used fraction: how far want has to move for its rounding to be got (to the midpoint between got and its bf16 neighbour
        # on want's side; 0 where got is bf16(want) itself), over the bound
        bits = B.bf16_bits(f32(g)).astype(np.int32)
        nb = f64(B.bf16_from_bits(np.clip(bits + np.where(np.abs(w) > np.abs(g), 1, -1), 0, 0xFFFF).astype(np.uint16))).reshape(g.shape)
        need = np.where(g == bf16_round64(w), 0.0, np.abs(w - np.where(g == 0, 0.0, 0.5 * (g + nb))))
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(need == 0, 0.0, need / b)
        with open(rec, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{float(np.nanmax(np.abs(g - w))):.3e}\t"
                    f"{float(np.nanmax(frac)):.3e}\tbf16-of-bounded\t{float(b.max()):.3e}\n")
    bad = ~((g >= lo) & (g <= hi))
    if bad.any():
        i = int(np.argmax(np.where(bad, np.where(np.isnan(g), np.inf, np.abs(g - w)), -1.0)))
        raise AssertionError(f"{what}: {int(bad.sum())}/{g.size} outside; worst got {g.flat[i]:.9e} want {w.flat[i]:.9e} "
                             f"(allowed [{lo.flat[i]:.9e}, {hi.flat[i]:.9e}], bound {b.flat[i]:.3e})")


def compare(got, want, what):
    """got: name -> array; want: name -> (float64, bound).  The one comparator of the CPU and the GPU tests."""
    for k, v in want.items():
        if not isinstance(v, tuple):
            continue
        if k.startswith(BF16_ONLY):
            assert k in got, f"{what}: {k} not produced"
            assert_bf16_of_bounded(got[k], v[0], v[1], f"{what} {k}")
            continue
        sh = shadow_of(k)
        assert k in got or sh in got, f"{what}: {k} not produced"
        if k in got:
            assert_bounded(got[k], v[0], v[1], f"{what} {k}")
            if sh in got:
                assert_bits_equal(got[sh], B.bf16_round(f32(got[k])), f"{what} {sh} against bf16({k})")
        else:
            assert_bf16_of_bounded(got[sh], v[0], v[1], f"{what} {sh}")


def has(c, k):
    """is output k written in case c?"""
    if c["op"] == "pool":
        return True
    if k.startswith("pooled_h_"):
        return "pooled_h" not in c["null"]
    if k.startswith("out_"):
        return "out" not in c["null"]
    if k.startswith("outh_"):
        return "out_h" not in c["null"]
    if k.startswith(("dl1h_", "dl2h_")):
        return c["dlh"]
    return True


def visible(c, full):
    """the outputs case c writes, of a complete set"""
    return {k: v for k, v in full.items() if has(c, k)}


def rounded(c, R):
    """a float64 result as a device would store it: fp32, the bf16 tensors rounded to bf16, the shadows beside them"""
    out = {}
    for k, v in R.items():
        if not isinstance(v, tuple):
            continue
        a = f32(v[0])
        out[k] = B.bf16_round(a) if k.startswith(BF16_ONLY) else a
        sh = shadow_of(k)
        if sh:
            out[sh] = B.bf16_round(a)
    return visible(c, out)


def saved_fwd(c, got, fill=None):
    """the S of ref_mid_fwd / ref_pool_fwd from a flat result; outputs the case leaves NULL come from `fill` (the same launch with
    every output present)"""
    src = dict(fill or {}, **got)
    if c["op"] == "pool":
        return dict(probs=[src[f"probs_{g}"] for g in range(len(c["sels"]))])
    ne1, ng1, ne2, ng2 = c["counts"]
    return dict(probs1=[src[f"probs1_{g}"] for g in range(ng1)], pooled_h=[src[f"pooled_h_{g}"] for g in range(ng1)], ex2=src["ex2"],
                probs2=[src[f"probs2_{t}"] for t in range(ng2)])


def saved_bwd(c, got):
    return dict(dz2_h=got["dz2_h"], dl2=[got[f"dl2_{t}"] for t in range(c["counts"][3])])


# ------------------------------------------------------------------------------------------------------------------------
# the launches in fp32 / bf16 numpy, in the kernels' operation order: stands in for a device on the CPU
# ------------------------------------------------------------------------------------------------------------------------
def _softmax32(l):
    l = f32(l)
    with np.errstate(over="ignore"):
        e = np.exp(l - l.max(1, keepdims=True))
    s = np.zeros((l.shape[0], 1), np.float32)
    for j in range(l.shape[1]):
        s = s + e[:, j:j + 1]
    return e * (np.float32(1) / s)


def _pool32(p, x, sel, H):
    X = f32(x).reshape(x.shape[0], -1, H)
    acc = np.zeros((x.shape[0], H), np.float32)
    for j, e in enumerate(sel):
        acc = acc + f32(p)[:, j:j + 1] * X[:, e]
    return acc


def _dlogits32(p, DO, x, sel, H):
    X = f32(x).reshape(x.shape[0], -1, H)[:, sel, :]
    dp = (f32(DO)[:, None, :] * X).sum(2, dtype=np.float32)
    dot = np.zeros((x.shape[0], 1), np.float32)
    for j in range(len(sel)):
        dot = dot + f32(p)[:, j:j + 1] * dp[:, j:j + 1]
    return f32(p) * (dp - dot)


def _expert_grad32(P, DO, sels, n_expert, H, x, mask, scale, old=None):
    n = x.shape[0]
    d = np.zeros((n, n_expert, H), np.float32)
    for e in range(n_expert):
        for g, sel in enumerate(sels):
            if e in sel:
                d[:, e] = d[:, e] + f32(P[g])[:, sel.index(e)][:, None] * f32(DO[g])
    if mask:
        d = np.where(f32(x).reshape(n, n_expert, H) > 0, d * np.float32(scale), np.float32(0))
    d = d.reshape(n, -1)
    return f32(old) + d if old is not None else d


def kernel32(c, D):
    """every output of the forward and of the backward launch of case c (complete: visible() drops what the case leaves NULL)"""
    got = {}
    if c["op"] == "pool":
        for g, sel in enumerate(c["sels"]):
            got[f"probs_{g}"] = _softmax32(D["logits"][g])
            got[f"out_{g}"] = _pool32(got[f"probs_{g}"], D["ex"], sel, c["H"])
        I = pool_bwd_inputs(c, D)
        for g, sel in enumerate(c["sels"]):
            got[f"dl_{g}"] = _dlogits32(I["probs"][g], D["dout"][g], D["ex"], sel, c["H"])
        got["dex"] = _expert_grad32(I["probs"], D["dout"], c["sels"], c["n_expert"], c["H"], D["ex"], c["mask"], c["scale"],
                                    D["dex0"] if c["acc"] else None)
    else:
        ne1, ng1, ne2, ng2 = c["counts"]
        T, n = c["topo"], c["B"]
        ks = keep_scale(c["p"])
        for g in range(ng1):
            got[f"probs1_{g}"] = _softmax32(D["logits1"][g])
            got[f"pooled_h_{g}"] = B.bf16_round(_pool32(got[f"probs1_{g}"], D["ex1"], T["sel1"][g], H1))
        ex2 = np.zeros((n, ne2, H2), np.float32)
        for e in range(ne2):
            z = f32(got[f"pooled_h_{T['src_e'][e]}"] @ f32(D["W"][e]).T)
            if c["bias"]:
                z = z + D["b"][e]
            if c["relu"]:
                z = np.maximum(z, np.float32(0))
            if c["p"] > 0:
                z = np.where(drop_keep(c, e), z * ks, np.float32(0))
            ex2[:, e] = z
        got["ex2"] = ex2.reshape(n, -1)
        for t in range(ng2):
            z = f32(got[f"pooled_h_{T['src_g'][t]}"] @ f32(D["Wg"][t]).T)
            if c["bias"]:
                z = z + D["bg"][t]
            got[f"probs2_{t}"] = _softmax32(z)
            got[f"out_{t}"] = _pool32(got[f"probs2_{t}"], got["ex2"], T["sel2"][t], H2)
        I = bwd_inputs(c, D)
        got["dz2_h"] = B.bf16_round(_expert_grad32(I["probs2"], D["dout"], T["sel2"], ne2, H2, I["ex2"], c["mask2"], c["scales"][1]))
        dl2h = []
        for t in range(ng2):
            got[f"dl2_{t}"] = _dlogits32(I["probs2"][t], D["dout"][t], I["ex2"], T["sel2"][t], H2)
            dl2h.append(B.bf16_round(got[f"dl2_{t}"]))
        dz = got["dz2_h"].reshape(n, ne2, H2)
        dP = []
        for s in range(ng1):
            v = np.zeros((n, H1), np.float32)
            for kind, i, h in k_steps(c, s):
                a, w = (dz[:, i, 32 * h:32 * h + 32], f32(D["W"][i])[32 * h:32 * h + 32]) if kind == "e" else (dl2h[i], f32(D["Wg"][i]))
                v = v + f32(a @ w)
            dP.append(v)
        got["dz1_h"] = B.bf16_round(_expert_grad32(I["probs1"], dP, T["sel1"], ne1, H1, D["ex1"], c["mask1"], c["scales"][0]))
        for g in range(ng1):
            got[f"dl1_{g}"] = _dlogits32(I["probs1"][g], dP[g], D["ex1"], T["sel1"][g], H1)
    for k in list(got):
        sh = shadow_of(k)
        if sh:
            got[sh] = B.bf16_round(got[k])
    return got


# ------------------------------------------------------------------------------------------------------------------------
# the scalar fields of the argument blocks (cdcmdr_amd._lib) from a case; pointers and strides are the test's
# ------------------------------------------------------------------------------------------------------------------------
def _set_sel(G, sel):
    G.n_sel = len(sel)
    for j, e in enumerate(sel):
        G.sel[j] = e


def mid_fwd_args(a, c):
    T = c["topo"]
    a.B, a.H1, a.H2 = c["B"], H1, H2
    a.n_exp1, a.n_gate1, a.n_exp2, a.n_gate2 = c["counts"]
    a.relu, a.drop_p, a.seed = c["relu"], c["p"], SEED
    for g, sel in enumerate(T["sel1"]):
        _set_sel(a.g1[g], sel)
    for e, s in enumerate(T["src_e"]):
        a.e2[e].src, a.e2[e].stream_id = s, c["stream_id"][e]
    for t, sel in enumerate(T["sel2"]):
        _set_sel(a.g2[t], sel)
        a.g2[t].src = T["src_g"][t]
    return a


def mid_bwd_args(a, c):
    T = c["topo"]
    a.B, a.H1, a.H2 = c["B"], H1, H2
    a.n_exp1, a.n_gate1, a.n_exp2, a.n_gate2 = c["counts"]
    a.mask1, a.mask2 = c["mask1"], c["mask2"]
    a.scale1, a.scale2 = c["scales"]
    for g, sel in enumerate(T["sel1"]):
        _set_sel(a.g1[g], sel)
    for e, s in enumerate(T["src_e"]):
        a.e2[e].src = s
    for t, sel in enumerate(T["sel2"]):
        _set_sel(a.g2[t], sel)
        a.g2[t].src = T["src_g"][t]
    return a


def pool_args(a, c):
    """cdc_pool_fwd_args or cdc_pool_bwd_args"""
    a.n_gates, a.n_expert, a.H, a.B = len(c["sels"]), c["n_expert"], c["H"], c["B"]
    if hasattr(a, "mask_relu"):
        a.mask_relu, a.mask_scale, a.accumulate = c["mask"], c["scale"], c["acc"]
    for g, sel in enumerate(c["sels"]):
        _set_sel(a.gate[g], sel)
    return a
