"""float64 restatements of the attention core (csrc/attention.hip), the factorisation-machine term and the row dot products
(csrc/rowops.hip), every value with a DERIVED error bound, for tests/test_gpu_attention.py, tests/test_gpu_fm.py and
tests/test_gpu_rowdot.py.  No GPU: tests/test_interaction_ref_cpu.py holds this file to torch float64 autograd.

The bounds, from the kernels' arithmetic (the library is built with -ffp-contract=off; U24 = 2^-24, one fp32 rounding):
  * a sum of n fp32 terms formed in any order takes at most n - 1 roundings of partial sums no larger than sum |term_i|
    (additions of 0 are exact), the products one more: helpers.sum_bound(sum |term_i|, n, c) with c further roundings;
  * attention scores: q dh^-1/2 is one rounding and rsqrtf's error (RSQRT_ULPS), then a dot product of dh terms;
  * softmax: exp(s_j - m) is shift invariant, so the fp32 maximum's own error cancels; what remains in the exponent is the score's
    error and the subtraction's rounding, an absolute error that becomes a relative one of e_j; numerator and denominator each
    carry the worst of these, the F additions, the reciprocal and the product one rounding each;
  * the backward takes the SAVED fp32 probabilities as its input (they are compared on their own), so its bounds hold only the
    backward's roundings: dP a dot product of dh terms, the row dot of F, dS three more, dQ / dK / dV sums of F terms;
  * FM: the per-dimension terms are (sum_f e)^2 and sum_f e^2, which cancel to 0 at F = 1: the bound is taken on those, not on |out|;
  * row dot: a dot product of K terms, the bias and the addends one rounding each; the sigmoid's own error is measured on the
    host against float64 (helpers.host_ulps) and allowed four times over, like the other transcendental kernels of the suite;
  * outputs are capped by OUT_FIG, cross-row sums by SUM_FIG, the attention's gradients by DQKV_FIG (helpers.capped)."""
import numpy as np

import bn_ref
from helpers import OUT_FIG, SUM_FIG, U24, capped, host_ulps, sum_bound, ulp32

DQKV_FIG = (2e-5, 2e-6)                       # tests/test_gpu_models_golden.py::test_attention_core_against_torch, d qkv
RSQRT_ULPS = 2                                # rsqrtf: 1 ulp documented, in units of 2^-24 relative at most 2
MUL = 0xD1342543DE82EF95                      # csrc/attention.hip: seed + uint32(step) * MUL
f64 = lambda a: np.asarray(a, dtype=np.float64)
f32 = lambda a: np.asarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
def attn_keep_mask(seed, step, B, H, F, p):
    """[B, H, F, F] bool: cdc_uniform(seed + uint32(step) MUL, ((b H + h) F + i) F + j) >= p keeps (step None: the NULL pointer)."""
    if p <= 0:
        return np.ones((B, H, F, F), dtype=bool)
    return bn_ref.keep_mask_uniform(seed, step, -64, np.arange(B * H * F), F, p).reshape(B, H, F, F)


def _heads(a, B, F, H, dh):
    """[B F, H dh] -> [B, H, F, dh]"""
    return f64(a).reshape(B, F, H, dh).transpose(0, 2, 1, 3)


def _rows(a, B, F, H, dh):
    """[B, H, F, dh] -> [B F, H dh]"""
    return a.transpose(0, 2, 1, 3).reshape(B * F, H * dh)


def _exp_ulps(arg64):
    """4 x what fp32 exp costs on the host over these arguments against float64, in ulps of the result"""
    a32 = f32(arg64)
    return 4 * host_ulps(np.exp(a32), np.exp(f64(a32)))


def attn_forward(qkv, B, F, A, H, keep, p):
    """qkv [B F, 3A] fp32, keep [B, H, F, F] bool, p the dropout probability (keep scale 1 / (1 - p)).
    Returns name -> (want, bound): probs [B, H, F, F] (before dropout), out [B F, A]; and the absolute-value sums under "abs"."""
    dh = A // H
    q, k, v = (_heads(qkv[:, i * A:(i + 1) * A], B, F, H, dh) for i in range(3))
    scale = dh ** -0.5
    s = np.einsum("bhid,bhjd->bhij", q, k) * scale
    a_s = np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k)) * scale
    e_s = sum_bound(a_s, dh, 1 + RSQRT_ULPS)
    m = s.max(-1, keepdims=True)
    arg = s - m
    e = np.exp(arg)
    probs = e / e.sum(-1, keepdims=True)
    # relative error of e_j: the exponent's absolute error (score, subtraction; the maximum lies within e_s of the true one, which
    # moves |s_j - m| by that much) and exp's own
    d_arg = e_s + U24 * (np.abs(arg) + e_s.max(-1, keepdims=True))
    rel_e = d_arg.max(-1, keepdims=True) + _exp_ulps(arg) * 2 * U24
    rel_p = 2 * rel_e + (F + 2) * U24
    rel_p = rel_p * (1 + rel_p)                                               # (second order)
    ks = 1.0 / (1.0 - p) if p > 0 else 1.0
    pd = probs * keep * ks
    out = np.einsum("bhij,bhjd->bhid", pd, v)
    a_out = np.einsum("bhij,bhjd->bhid", np.abs(pd), np.abs(v))
    b_out = (rel_p + (F + 2) * U24) * a_out
    return {"probs": (probs, capped(rel_p * probs, probs, OUT_FIG)),
            "out": (_rows(out, B, F, H, dh), capped(_rows(b_out, B, F, H, dh), _rows(out, B, F, H, dh), OUT_FIG)),
            "abs": {"scores": a_s, "out": _rows(a_out, B, F, H, dh)}}


def attn_backward(qkv, probs, dout, B, F, A, H, keep, p):
    """The gradient of sum(out * dout) with respect to qkv, from the given probabilities (the forward's saved fp32 values in a GPU
    test, float64 ones in the CPU test).  Returns name -> (want, bound) for dq, dk, dv [B F, A] each, and "abs"."""
    dh = A // H
    q, k, v = (_heads(qkv[:, i * A:(i + 1) * A], B, F, H, dh) for i in range(3))
    do, P = _heads(dout, B, F, H, dh), f64(probs)
    scale = dh ** -0.5
    ks = 1.0 / (1.0 - p) if p > 0 else 1.0
    kk = keep * ks
    dp = np.einsum("bhid,bhjd->bhij", do, v) * kk
    a_dp = np.einsum("bhid,bhjd->bhij", np.abs(do), np.abs(v)) * kk
    e_dp = sum_bound(a_dp, dh, 1)
    dot = (dp * P).sum(-1, keepdims=True)
    a_dot = (np.abs(dp) * P).sum(-1, keepdims=True)
    e_dot = (e_dp * P).sum(-1, keepdims=True) + sum_bound(a_dot, F, 0)
    ds = P * (dp - dot)
    e_ds = P * (e_dp + e_dot) + 2 * U24 * P * (np.abs(dp) + np.abs(dot))
    qs = q * scale
    pd = P * kk
    dq = np.einsum("bhij,bhjd->bhid", ds, k) * scale
    b_dq = scale * (np.einsum("bhij,bhjd->bhid", e_ds, np.abs(k)) + sum_bound(np.einsum("bhij,bhjd->bhid", np.abs(ds), np.abs(k)), F, 0)) + \
        (1 + RSQRT_ULPS) * U24 * np.abs(dq)
    dk = np.einsum("bhij,bhid->bhjd", ds, qs)
    a_dk = np.einsum("bhij,bhid->bhjd", np.abs(ds), np.abs(qs))
    b_dk = np.einsum("bhij,bhid->bhjd", e_ds, np.abs(qs)) + sum_bound(a_dk, F, 1 + RSQRT_ULPS)
    dv = np.einsum("bhij,bhid->bhjd", pd, do)
    a_dv = np.einsum("bhij,bhid->bhjd", np.abs(pd), np.abs(do))
    b_dv = sum_bound(a_dv, F, 1)
    R = {"abs": {"dp": a_dp, "dk": _rows(a_dk, B, F, H, dh), "dv": _rows(a_dv, B, F, H, dh)}}
    for nm, w, b in (("dq", dq, b_dq), ("dk", dk, b_dk), ("dv", dv, b_dv)):
        w2 = _rows(w, B, F, H, dh)
        R[nm] = (w2, capped(_rows(b, B, F, H, dh), w2, DQKV_FIG))
    return R


# ------------------------------------------------------------------------------------------------------------------------
# the second-order factorisation-machine term: out[b] = 1/2 sum_d ((sum_f e[b,f,d])^2 - sum_f e[b,f,d]^2)
# ------------------------------------------------------------------------------------------------------------------------
def fm_forward(e, F, D):
    """e [B, F D] fp32.  Returns (want [B], bound [B])."""
    x = f64(e).reshape(-1, F, D)
    s, S, Q = x.sum(1), np.abs(x).sum(1), (x * x).sum(1)
    want = 0.5 * (s * s - Q).sum(1)
    # per dimension: s takes F roundings of at most S; its square 2 F + 1 of S^2; q takes F + 1 of Q; the difference one of both.
    # Over the dimensions: a lane's trips and the six steps of the butterfly.  The factor 1/2 is exact.
    n = (2 * F + 2) + (D + 63) // 64 + 6
    return want, capped(0.5 * n * U24 * (S * S + Q).sum(1), want, OUT_FIG)


def fm_backward(e, dout, F, D, old=None):
    """de[b,f,d] (+)= dout[b] (sum_f' e[b,f',d] - e[b,f,d]); old: the accumulate target's values.  Returns (want, bound) [B, F D]."""
    x = f64(e).reshape(-1, F, D)
    g = f64(dout).reshape(-1, 1, 1)
    s, S = x.sum(1, keepdims=True), np.abs(x).sum(1, keepdims=True)
    v = g * (s - x)
    b = np.abs(g) * (F + 1) * U24 * (S + np.abs(x)) + U24 * np.abs(v)
    want = v.reshape(-1, F * D)
    b = b.reshape(-1, F * D)
    if old is not None:
        want = want + f64(old)
        b = b + U24 * (np.abs(f64(old)) + np.abs(v.reshape(-1, F * D)))
    return want, capped(b, want, OUT_FIG)


# ------------------------------------------------------------------------------------------------------------------------
# row dot products: out[b] = sigmoid?(x[b, :] . w + bias + sum_i addend_i[b])
# ------------------------------------------------------------------------------------------------------------------------
def _sig32(z32):
    with np.errstate(over="ignore"):
        return np.float32(1) / (np.float32(1) + np.exp(-f32(z32)))


def rowdot_forward(x, w, bias, addends, sigmoid):
    """x [M, K], w [K], bias a float or None, addends a list of [M].  Returns {"logit": (want, bound), "out": (want, bound)}."""
    x, w = f64(x), f64(w)
    M, K = x.shape
    z, a = x @ w, np.abs(x) @ np.abs(w)
    extra = 0
    if bias is not None:
        z, a, extra = z + float(bias), a + abs(float(bias)), extra + 1
    for ad in addends:
        z, a, extra = z + f64(ad), a + np.abs(f64(ad)), extra + 1
    b_z = sum_bound(a, K, extra)
    R = {"logit": (z, capped(b_z, z, OUT_FIG))}
    if sigmoid:
        o = 1.0 / (1.0 + np.exp(-z))
        ulps = 4 * host_ulps(_sig32(z), 1.0 / (1.0 + np.exp(-f64(f32(z)))))
        R["out"] = (o, capped(b_z * o * (1.0 - o) * (1 + b_z) + ulps * ulp32(o), o, OUT_FIG))
    else:
        R["out"] = R["logit"]
    return R


def rowdot_backward(x, w, dout, out32, sigmoid, dx_old=None):
    """The plain backward of one group over its own rows: d = dout (out (1 - out) with the sigmoid, from the fp32 outputs given);
    dlogit = d, dx (+)= d w, dw = sum_rows d x, dbias = sum_rows d.  Returns name -> (want, bound)."""
    x, w, d = f64(x), f64(w), f64(dout).reshape(-1)
    M, K = x.shape
    cd = 0
    if sigmoid:
        o = f64(out32).reshape(-1)
        d = d * o * (1.0 - o)
        cd = 3                                                                # d o, 1 - o, their product
    ad = np.abs(d)
    v = d[:, None] * w[None, :]
    b_dx = (cd + 1) * U24 * np.abs(v)
    dx = v
    if dx_old is not None:
        dx = v + f64(dx_old)
        b_dx = b_dx + U24 * (np.abs(f64(dx_old)) + np.abs(v))
    dw, db = d @ x, d.sum()
    return {"dlogit": (d.reshape(M, 1), capped(cd * U24 * ad, d, OUT_FIG).reshape(M, 1)),
            "dx": (dx, capped(b_dx, dx, OUT_FIG)),
            "dw": (dw.reshape(1, K), capped(sum_bound(ad @ np.abs(x), M, cd + 1), dw, SUM_FIG).reshape(1, K)),
            "dbias": (np.array([[db]]), capped(sum_bound(ad.sum(), M, cd), db, SUM_FIG).reshape(1, 1))}
