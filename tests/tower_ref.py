"""float64 restatement of what include/cdcmdr.h promises for cdc_tower_args (cdc_tower_fwd / _bwd / _step / _dp of
csrc/tower.hip), every value with a DERIVED error bound, an fp32 / bf16 restatement in the kernels' operation order that stands in
for a device on the CPU, the launches tests/test_gpu_tower_direct.py runs, and the seeded defects the bounds have to reject.  No
GPU: tests/test_tower_ref_cpu.py holds this file, tests/test_gpu_tower_direct.py holds the launches to it.

The chain is discontinuous (bf16 roundings of a1h and dzh, ReLU, dropout), so the reference is STAGE-WISE: every stage is computed
in float64 from the tensors the launch itself saved for the stage before (`S`: z1, a1h, z2, a2, out, the saved statistics, dzh2,
dzh1), as tests/test_gpu_head.py and tests/bn_ref.py do.  With S = None the stages are chained on their own float64 results
(nothing rounded): that composition is what tests/test_tower_ref_cpu.py holds against torch autograd.

Every ref_* function returns name -> (want, bound); per-tower names end in the tower's index ("z1_0", "dgamma2_1").

The bounds, from the kernels' arithmetic (the library is built with -ffp-contract=off):
  * z1, z2, dx and the unobservable dA1 are bf16 MFMA contractions: products of bf16 operands are exact in fp32, so
    sum_bound(sum |a_i b_i|, n = K, c) with c = 1 for the bias resp. the += of accumulate_dx — glinear_ref.ref_fwd / ref_bwdx on
    the operand bits, capped by glinear_ref.Y_FIG / G_FIG.  The MFMA's summation order is not known: NO allowance beyond that c.
    Measured on an MI355X (profiles/tower_margins.txt, one clean run of the whole module): z1 uses at most 0.031 of its bound,
    z2 0.034, dx 0.054 — the bf16 MFMA needs no allowance of its own;
  * the BatchNorm stages are bn_ref.ref_forward / ref_backward (fp64 column sums with the U53 accounting there: the towers' chunk
    and block sums have at most chunks + 24 double roundings), a1h and dzh with bn_ref.bf16_half_ulp on top; the dropout stream is
    bn_ref.keep_mask_bits16(seed1 | seed2, step, tower, ...);
  * the logit gradient d takes 3 roundings (d_out o (1 - o)), + 7 in the fused-BCE form (tests/test_gpu_head.py's count); the
    gradient handed to a BatchNorm's backward carries them (+ 1 for the product with wo), dA1 carries its contraction's bound:
    bn_ref.ref_backward(ddy=...) joins that to every bound downstream;
  * dwo / dbo: fp32 products summed in double per block, one fp32 value per block, the blocks added in fp32: n = blocks, c = the
    roundings of d + 2; wide_dw / wide_dbias: a wave adds at most 32 rows in fp32, four waves, then at most 4 + 6 additions over
    the workgroups' partials: n = min(M, 32) + 13 + n_tower; capped by SUM_FIG;
  * out: n = H2 + wide_K + 1 products and c = 3 roundings on the logit, carried through the sigmoid with test_gpu_head's
    allowance for expf (4 x the ulps the host's fp32 evaluation measures: SIGMOID_ULPS_HOST); capped by OUT_FIG and, for
    probabilities, by the 2e-6 of tests/test_gpu_tower.py; the loss as in tests/test_gpu_head.py.
Nothing is looser than the suite's present figures (helpers.capped).

The activation mask of the backward is the SIGN of the saved activation, as everywhere in this library ("only its sign is
used", cdc_bn_bwd_args): with relu = 0 AND dropout a kept negative value would lose its gradient, so relu = 0 runs without dropout
here, as it does in every model."""
import numpy as np

import bn_ref as B
import glinear_ref as GL
from helpers import OUT_FIG, SUM_FIG, U24, capped, host_ulps, sum_bound, ulp32

H1, H2, ROWS = 64, 32, 128                      # the instantiated hidden sizes, CDC_TOWER_ROWS
SEED1, SEED2 = 0x1234_5678_9ABC_DEF1, 0x0FED_CBA9_8765_4321
PROB_FIG = (0.0, 2e-6)                          # tests/test_gpu_tower.py, probabilities
EPS, MOMENTUM = 1e-5, 0.1
# 1 / (1 + expf(-z)) and the loss terms in fp32 on the host against float64, in ulps of the result, worst over the cases of this
# file: 2.93 at the 16512 x 1 and 8192 x 4 logits, 3.43 for the loss terms of rows127_bce (tests/test_gpu_head.py has 2.6 and 2.4
# over fewer rows); allowed: 4 x, the device's expf / logf need not match the host's last bits
SIGMOID_ULPS_HOST, LOSS_ULPS_HOST = 3.0, 3.5
NULLABLE = ("dgamma", "dbeta", "dwo", "dbo", "dx", "wide_dx", "wide_dw", "wide_dbias")
f64 = lambda a: np.asarray(a, dtype=np.float64)
f32 = lambda a: np.asarray(a, dtype=np.float32)

DEFECTS = ("stats_drop_last_row", "biased_running_var", "drop2_from_seed1", "drop_stream_tower0", "seed_offset_ignored",
           "mask_from_z", "no_mask_scale", "block_M", "loss_all_towers", "group_unclamped", "wide_two_towers", "wide_no_tower",
           "acc_dx_off", "acc_wide_off", "no_bo", "operand_unrounded")
FWD_DEFECTS = ("stats_drop_last_row", "biased_running_var", "drop2_from_seed1", "drop_stream_tower0", "seed_offset_ignored", "no_bo",
               "operand_unrounded")


# ------------------------------------------------------------------------------------------------------------------------
# launch descriptions
# ------------------------------------------------------------------------------------------------------------------------
def case(name, M, n_tower=3, H0=64, relu=1, sigmoid=1, p=0.2, step=5, wide=28, wide_bias=True, bo=True, running=True, nbt=True,
         form="dout", group="rand", acc_dx=None, acc_wide=0, null=(), data="normal"):
    """form: "dout" (the output gradient comes from outside) | "i16" | "f32" (fused BCE on int16 / float labels).
    group: "rand" | "none" (bce_group NULL) | "outside" (-1 and n_tower among valid ones) | "one" (every row in tower 1).
    step: the value behind seed_offset_dev, None = NULL.  wide: wide_K, 0 = no wide term.  null: output pointers left NULL
    (in every tower).  data: "normal" | "degen" (a zero row of W1 with zero bias, a zero gamma per layer, a zero wo element) |
    "extreme" (bo = 40, -40, -110: outputs exactly 1, 4e-18 and 0, both clamps of the loss and the 1e-12 floor act)."""
    assert form in ("dout", "i16", "f32") and group in ("rand", "none", "outside", "one") and set(null) <= set(NULLABLE)
    assert not (relu == 0 and p > 0), "see the module docstring"
    return dict(name=name, M=M, n_tower=n_tower, H0=H0, relu=relu, sigmoid=sigmoid, p=p, step=step, wide=wide, wide_bias=wide_bias, bo=bo,
                running=running, nbt=nbt, form=form, group=group, acc_dx=tuple(acc_dx) if acc_dx else (0,) * n_tower, acc_wide=acc_wide,
                null=tuple(null), data=data)


def bce(c):
    return c["form"] != "dout"


def scalar_args(a, c):
    """the scalar fields of a cdc_tower_args (cdcmdr_amd._lib.TowerArgs) from a case; pointers and strides are the test's"""
    a.n_tower, a.H0, a.H1, a.H2, a.M = c["n_tower"], c["H0"], H1, H2, c["M"]
    a.relu, a.sigmoid, a.drop_p, a.eps, a.momentum = c["relu"], c["sigmoid"], c["p"], EPS, MOMENTUM
    a.seed1, a.seed2 = SEED1, SEED2
    a.wide_K, a.accumulate_wide_dx = c["wide"], c["acc_wide"]
    a.bce_inv_count = inv_count(c) if bce(c) else 0.0
    for t in range(c["n_tower"]):
        a.t[t].accumulate_dx = c["acc_dx"][t]
    return a


def cases():
    S = []
    for M in (2, 63, 64, 65, 127, 128, 129, 193, 257):          # chunk and block boundaries, a one-row last block, odd chunk counts
        S.append(case(f"rows{M}_dout", M))
        S.append(case(f"rows{M}_bce", M, form="i16"))
    S += [case("h128_65", 65, H0=128, form="i16"), case("h128_257", 257, H0=128, acc_dx=(0, 1, 0)),
          case("nt1", 129, n_tower=1, form="i16"), case("nt2", 129, n_tower=2), case("nt4", 129, n_tower=4, form="f32"),
          case("relu0", 129, relu=0, p=0.0), case("nosig", 129, sigmoid=0), case("p0", 129, p=0.0, form="i16"),
          case("p05", 129, p=0.5), case("nostep", 129, step=None, form="i16"), case("nobo", 129, bo=False, form="i16"),
          case("norun", 129, running=False), case("nonbt", 129, nbt=False, form="i16"),
          case("accdx", 129, acc_dx=(1, 0, 1), form="i16"), case("accwide", 129, acc_wide=1), case("accwide_bce", 129, acc_wide=1, form="i16")]
    S += [case(f"null_{k}", 65, null=(k,), form="i16" if i % 2 else "dout") for i, k in enumerate(NULLABLE)]
    S += [case("wide0", 129, wide=0, form="i16"), case("wide4", 129, wide=4), case("wide256", 129, wide=256, form="i16"),
          case("wide260", 129, wide=260), case("wide512", 129, wide=512, form="i16", acc_wide=1), case("nowb", 129, wide_bias=False)]
    S += [case("bce_f32", 129, form="f32"), case("bce_nogroup", 129, form="i16", group="none"),
          case("bce_outside", 129, form="f32", group="outside"), case("bce_outside16", 65, form="i16", group="outside"), case("bce_one", 257, form="i16", group="one", wide=260),
          case("extreme", 129, form="f32", data="extreme"), case("extreme_dout", 65, data="extreme"),
          case("degen", 129, data="degen", form="i16"), case("degen_dout", 65, data="degen", p=0.0)]
    # the gather loops (one tower: the row counts stay within 256 workgroups) and the residency limit
    S += [case("gather4160", 4160, n_tower=1, wide=4), case("gather16512", 16512, n_tower=1, form="i16", wide=28),
          case("resident256", 8192, n_tower=4, form="i16", wide=260)]
    assert len({c["name"] for c in S}) == len(S)
    return S


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def make_data(c):
    """seeded by the case's name; x, W1, W2 hold bf16-representable values (the test writes their bits)"""
    rng = _rng(c["name"])
    M, n, H0, K = c["M"], c["n_tower"], c["H0"], c["wide"]
    D = dict(x=[], W1=[], b1=[], g1=[], be1=[], rm1=[], rv1=[], nbt1=[], W2=[], b2=[], g2=[], be2=[], rm2=[], rv2=[], nbt2=[], wo=[], bo=[],
             dx0=[])
    for t in range(n):
        D["x"].append(B.bf16_round(f32(rng.standard_normal((M, H0)))))
        D["W1"].append(B.bf16_round(f32(rng.standard_normal((H1, H0)) / np.sqrt(H0))))
        D["W2"].append(B.bf16_round(f32(rng.standard_normal((H2, H1)) / np.sqrt(H1))))
        for l, C in ((1, H1), (2, H2)):
            D[f"b{l}"].append(f32(0.3 * rng.standard_normal(C)))
            D[f"g{l}"].append(f32(rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)))
            D[f"be{l}"].append(f32(0.3 * rng.standard_normal(C)))
            D[f"rm{l}"].append(f32(rng.standard_normal(C)))
            D[f"rv{l}"].append(f32(rng.uniform(0.5, 2.0, C)))
            D[f"nbt{l}"].append(int(rng.integers(0, 1000)))
        D["wo"].append(f32(rng.standard_normal(H2) / np.sqrt(H2)))
        D["bo"].append(f32(0.3 * rng.standard_normal(1)) if c["bo"] else None)
        D["dx0"].append(f32(rng.standard_normal((M, H0))))
        if c["data"] == "degen":
            D["W1"][t][5], D["b1"][t][5] = 0.0, 0.0              # z1[:, 5] == 0: sums exactly 0, invstd = eps^-1/2, a1 = relu(beta)
            D["g1"][t][7], D["g2"][t][3], D["wo"][t][2] = 0.0, 0.0, 0.0
    if c["data"] == "extreme":
        for t, v in zip(range(n), (40.0, -40.0, -110.0)):
            D["bo"][t] = f32([v])
    if K:
        D.update(wx=f32(rng.standard_normal((M, K))), ww=f32(rng.standard_normal(K) / np.sqrt(K)),
                 wb=f32(0.3 * rng.standard_normal(1)) if c["wide_bias"] else None, wdx0=f32(rng.standard_normal((M, K))))
    D["dout"] = f32(rng.standard_normal((M, n)))
    y = rng.integers(0, 2, size=M)
    if c["form"] == "f32":
        y = np.where(rng.random(M) < 0.25, 0.3 + 0.4 * rng.random(M), y)        # soft labels: both terms of the loss at once
        y[:2] = (0.3, 1.0)
    D["y"] = y.astype(np.float32 if c["form"] == "f32" else np.int16)
    g = rng.integers(0, n, size=M).astype(np.int64)
    if c["group"] == "outside":
        g[::5], g[2::7] = -1, n
    if c["group"] == "one":
        g[:] = 1
    D["group"] = None if c["group"] == "none" else g
    return D


def own_tower(c, D, clamp=True):
    M, n = c["M"], c["n_tower"]
    own = np.zeros(M, dtype=np.int64) if D["group"] is None else D["group"].copy()
    if clamp:
        own[(own < 0) | (own >= n)] = 0
    return own


def inv_count(c):
    return float(np.float32(1.0) / np.float32(c["M"]))


def wide_owner(c, D):
    """the tower whose workgroup forms row r's wide gradient: the row's own tower (fused BCE), r % n_tower otherwise"""
    return own_tower(c, D) if bce(c) else np.arange(c["M"]) % c["n_tower"]


def _sig(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ------------------------------------------------------------------------------------------------------------------------
# the BatchNorm stages as bn_ref launches: segment t = tower t (dropout stream 64 + t), 16-byte family
# ------------------------------------------------------------------------------------------------------------------------
def bn_spec(c, layer, towers=None, defect=None):
    n = c["n_tower"] if towers is None else len(towers)
    seed = SEED1 if (layer == 1 or defect == "drop2_from_seed1") else SEED2
    step = None if defect == "seed_offset_ignored" else c["step"]
    return B.spec(f"{c['name']}.bn{layer}", (H1 if layer == 1 else H2,) * n, c["M"], pad=4, relu=c["relu"], eps=EPS, momentum=MOMENTUM,
                  drop_p=c["p"], step=step, seed=seed, running=c["running"], nbt=c["nbt"], y="h" if layer == 1 else "f", dx="h")


def bn_data(c, D, layer, Z, towers=None, dy=None):
    T = range(c["n_tower"]) if towers is None else towers
    l = str(layer)
    return dict(x=[Z[t] for t in T], gamma=[D["g" + l][t] for t in T], beta=[D["be" + l][t] for t in T], rm=[D["rm" + l][t] for t in T],
                rv=[D["rv" + l][t] for t in T], nbt=[D["nbt" + l][t] for t in T], dy=None if dy is None else [dy[t] for t in T],
                dx0=[None for _ in T])


def _bn_forward(c, D, layer, Z, defect):
    bd = defect if defect in ("stats_drop_last_row", "biased_running_var") else None
    if defect == "drop_stream_tower0":                              # every tower draws from stream 64 + 0
        return [B.ref_forward(bn_spec(c, layer, [t]), bn_data(c, D, layer, Z, [t]), bd)[0] for t in range(c["n_tower"])]
    return B.ref_forward(bn_spec(c, layer, defect=defect), bn_data(c, D, layer, Z), bd)


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
def _linear(name, x, w, b, K, N):
    cs = GL.fwd_case(name, K, x.shape[0], [N], relu=0)
    return GL.ref_fwd(cs, dict(x=x, w=[w], b=[b]), GL.BF16)["y0"]


def ref_forward(c, D, S=None, defect=None):
    """S: the launch's saved tensors (lists per tower: z1, a1h, z2, a2); None chains the stages on their own float64 results."""
    M, n, K = c["M"], c["n_tower"], c["wide"]
    chain = S is None
    R, W = {}, dict(z1=[], a1h=[], z2=[], a2=[], mean1=[], inv1=[], mean2=[], inv2=[])
    for t in range(n):
        R[f"z1_{t}"] = _linear("z1", D["x"][t], D["W1"][t], D["b1"][t], c["H0"], H1)
        W["z1"].append(R[f"z1_{t}"][0])
    src = W if chain else S
    bn1 = _bn_forward(c, D, 1, src["z1"], defect)
    for t in range(n):
        _bn_names(R, bn1[t], 1, t, "a1h", "yh", c)
        W["a1h"].append(bn1[t]["yh"][0]); W["mean1"].append(bn1[t]["save_mean"][0]); W["inv1"].append(bn1[t]["save_invstd"][0])
    for t in range(n):
        a1 = W["a1h"][t] if (chain or defect == "operand_unrounded") else f64(S["a1h"][t])
        if chain or defect == "operand_unrounded":                   # (nothing rounded: the float64 contraction itself)
            z = f64(a1) @ f64(D["W2"][t]).T + f64(D["b2"][t])
            R[f"z2_{t}"] = (z, capped(sum_bound(np.abs(f64(a1)) @ np.abs(f64(D["W2"][t])).T + np.abs(f64(D["b2"][t])), H1, 1), z, GL.Y_FIG))
        else:
            R[f"z2_{t}"] = _linear("z2", f32(a1), D["W2"][t], D["b2"][t], H1, H2)
        W["z2"].append(R[f"z2_{t}"][0])
    src = W if chain else S
    bn2 = _bn_forward(c, D, 2, src["z2"], defect)
    for t in range(n):
        _bn_names(R, bn2[t], 2, t, "a2", "y", c)
        W["a2"].append(bn2[t]["y"][0]); W["mean2"].append(bn2[t]["save_mean"][0]); W["inv2"].append(bn2[t]["save_invstd"][0])
    # the head: Linear(H2 -> 1) + bo + the wide term, sigmoid
    src = W if chain else S
    shared, a_shared = np.zeros(M), np.zeros(M)
    if K:
        shared, a_shared = f64(D["wx"]) @ f64(D["ww"]), np.abs(f64(D["wx"])) @ np.abs(f64(D["ww"]))
        if D["wb"] is not None:
            shared, a_shared = shared + float(D["wb"][0]), a_shared + abs(float(D["wb"][0]))
    z, dz = np.zeros((M, n)), np.zeros((M, n))
    for t in range(n):
        a2, wo = f64(src["a2"][t]), f64(D["wo"][t])
        acc, a_acc = a2 @ wo + shared, np.abs(a2) @ np.abs(wo) + a_shared
        if D["bo"][t] is not None and defect != "no_bo":
            acc, a_acc = acc + float(D["bo"][t][0]), a_acc + abs(float(D["bo"][t][0]))
        z[:, t], dz[:, t] = acc, sum_bound(a_acc, H2 + K + 1, 3)
    if not c["sigmoid"]:
        R["out"] = (z, capped(dz, z, OUT_FIG))
    else:
        out = _sig(z)
        z32 = z.astype(np.float32)
        with np.errstate(over="ignore"):
            host = np.float32(1) / (np.float32(1) + np.exp(-z32))
        R["sigmoid_ulps"] = host_ulps(host, _sig(z32.astype(np.float64)))
        prop = np.maximum(_sig(z + dz) - out, out - _sig(z - dz))
        R["out"] = (out, capped(capped(prop + 4 * SIGMOID_ULPS_HOST * ulp32(out), out, OUT_FIG), out, PROB_FIG))
    W["out"] = R["out"][0]
    R["chained"] = W
    return R


def _bn_names(R, b, layer, t, act, key, c):
    R[f"{act}_{t}"] = b[key]
    R[f"mean{layer}_{t}"], R[f"inv{layer}_{t}"] = b["save_mean"], b["save_invstd"]
    if c["running"]:
        R[f"rm{layer}_{t}"], R[f"rv{layer}_{t}"] = b["running_mean"], b["running_var"]
    if c["nbt"]:
        R[f"nbt{layer}_{t}"] = b["nbt"]


# ------------------------------------------------------------------------------------------------------------------------
# backward: from the saved z1, a1h, z2, a2, out and statistics (and the launch's own dzh bits for the two grad-input products)
# ------------------------------------------------------------------------------------------------------------------------
def logit_gradients(c, D, out, defect=None):
    """-> d [M, n_tower], its rounding count, and with the fused loss (loss, bound)"""
    M, n = c["M"], c["n_tower"]
    o = f64(out)
    cd, loss = 0, None
    if bce(c):
        y = f64(D["y"])
        own = own_tower(c, D)
        live = np.ones(M, dtype=bool)
        if defect == "group_unclamped" and D["group"] is not None:
            live = (D["group"] >= 0) & (D["group"] < n)
        inv = inv_count(c)
        sel = np.zeros((M, n), dtype=bool)
        sel[np.arange(M), own] = live
        if defect == "loss_all_towers":
            sel[:] = True
        yy = np.broadcast_to(y[:, None], (M, n))
        with np.errstate(divide="ignore", invalid="ignore"):
            la, lb = np.maximum(np.log1p(-o), -100.0), np.maximum(np.log(o), -100.0)
        rows = np.where(sel, (yy - 1.0) * la - yy * lb, 0.0)
        mag = np.where(sel, np.abs((yy - 1.0) * la) + np.abs(yy * lb), 0.0)
        o32, y32 = o.astype(np.float32), yy.astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            host = (y32 - np.float32(1)) * np.maximum(np.log1p(-o32), np.float32(-100)) - y32 * np.maximum(np.log(o32), np.float32(-100))
        ok = sel & (mag > 0)
        ulps = float(np.max(np.abs(host.astype(np.float64) - rows)[ok] / ulp32(mag)[ok])) if ok.any() else 0.0
        total = rows.sum() * inv
        loss = (np.array([total]), capped(np.array([inv * np.sum(4 * LOSS_ULPS_HOST * ulp32(mag)) + 2 * U24 * abs(total)]), total, OUT_FIG), ulps)
        dout = np.where(sel, inv * (o - yy) / np.maximum((1.0 - o) * o, 1e-12), 0.0)
        cd = 7
    else:
        dout = f64(D["dout"])
    d = dout * o * (1.0 - o) if c["sigmoid"] else dout
    cd += 3 if c["sigmoid"] else 0
    return d, cd, loss


def _grad_input(name, dz, w, K, N, old=None, defect=None):
    cs = GL.bwdx_case(name, dz.shape[0], [(K, None, int(old is not None))], [(N, 0)])
    return GL.ref_bwdx(cs, dict(dz=[dz], w=[w], dx0=[old], mask=[None]), GL.BF16, defect)["dx0"]


def ref_backward(c, D, S, defect=None, chain=False):
    """S: z1, a1h, z2, a2 (lists per tower), out, mean1 / inv1 / mean2 / inv2 and — unless chain — dzh2, dzh1."""
    M, n, K, H0 = c["M"], c["n_tower"], c["wide"], c["H0"]
    G = -(-M // ROWS)
    R = {}
    d, cd, loss = logit_gradients(c, D, S["out"], defect)
    if loss is not None:
        R["loss"], R["loss_ulps"] = loss[:2], loss[2]
    ad = np.abs(d)
    nul = set(c["null"])
    bdef = {"mask_from_z": "mask_from_x", "no_mask_scale": "no_mask_scale"}.get(defect)
    div = None
    if defect == "block_M":
        blk = np.minimum(ROWS, M - (np.arange(M) // ROWS) * ROWS).astype(np.float64)
        div = [blk] * n
    # ---- the head's parameters
    for t in range(n):
        a2 = f64(S["a2"][t])
        if "dwo" not in nul:
            v = d[:, t] @ a2
            R[f"dwo_{t}"] = (v, capped(sum_bound(ad[:, t] @ np.abs(a2), G, cd + 2), v, SUM_FIG))
        if "dbo" not in nul and c["bo"]:
            v = np.array([d[:, t].sum()])
            R[f"dbo_{t}"] = (v, capped(sum_bound(ad[:, t].sum(), G, cd + 1), v, SUM_FIG))
    # ---- BatchNorm 2: dy = d wo
    dy2 = [d[:, t:t + 1] * f64(D["wo"][t])[None, :] for t in range(n)]
    b2 = B.ref_backward(bn_spec(c, 2), bn_data(c, D, 2, S["z2"], dy=dy2), S["a2"], S["mean2"], S["inv2"], bdef,
                        ddy=[(cd + 1) * U24 * np.abs(v) for v in dy2], divisor=div)
    dz2w = [b2[t]["dxh"][0] for t in range(n)]
    # ---- dA1 = dZ2 W2 (not observable: its bound joins the next stage's), BatchNorm 1
    dy1, ddy1 = [], []
    for t in range(n):
        if chain or defect == "operand_unrounded":
            v = f64(dz2w[t]) @ f64(D["W2"][t])
            e = capped(sum_bound(np.abs(f64(dz2w[t])) @ np.abs(f64(D["W2"][t])), H2, 0), v, GL.G_FIG)
        else:
            v, e = _grad_input("dA1", f32(S["dzh2"][t]), D["W2"][t], H1, H2)
        dy1.append(v); ddy1.append(e)
    b1 = B.ref_backward(bn_spec(c, 1), bn_data(c, D, 1, S["z1"], dy=dy1), S["a1h"], S["mean1"], S["inv1"], bdef, ddy=ddy1, divisor=div)
    dz1w = [b1[t]["dxh"][0] for t in range(n)]
    for t in range(n):
        for l, b in ((2, b2), (1, b1)):
            R[f"dzh{l}_{t}"] = b[t]["dxh"]
            if "dgamma" not in nul:
                R[f"dgamma{l}_{t}"] = b[t]["dgamma"]
            if "dbeta" not in nul:
                R[f"dbeta{l}_{t}"] = b[t]["dbeta"]
        if "dx" not in nul:
            old = D["dx0"][t] if c["acc_dx"][t] else None
            if chain or defect == "operand_unrounded":
                v = f64(dz1w[t]) @ f64(D["W1"][t]) + (f64(old) if old is not None else 0.0)
                tm = np.abs(f64(dz1w[t])) @ np.abs(f64(D["W1"][t])) + (np.abs(f64(old)) if old is not None else 0.0)
                R[f"dx_{t}"] = (v, capped(sum_bound(tm, H1, int(old is not None)), v, GL.G_FIG))
            else:
                R[f"dx_{t}"] = _grad_input("dx", f32(S["dzh1"][t]), D["W1"][t], H0, H1, old, "acc_off" if defect == "acc_dx_off" else None)
    # ---- the wide term: every tower's logit gradient (fused BCE: the row's own tower alone, the others are zero)
    if K:
        dsum, a_dsum = d.sum(1), ad.sum(1)
        wx, ww = f64(D["wx"]), f64(D["ww"])
        times = np.ones(M)
        if defect == "wide_two_towers":
            times[::3] = 2.0
        if defect == "wide_no_tower":
            times[::3] = 0.0
        n_w = min(M, 32) + 13 + n
        if "wide_dx" not in nul:
            v = dsum[:, None] * ww[None, :]
            b = sum_bound(a_dsum[:, None] * np.abs(ww)[None, :], n, cd + 1)
            if c["acc_wide"] and defect != "acc_wide_off":
                v = f64(D["wdx0"]) + v * times[:, None]
                b = b + U24 * np.abs(v)
            v = np.where(times[:, None] > 0, v, np.nan if not c["acc_wide"] else f64(D["wdx0"]))
            R["wide_dx"] = (v, capped(b, v, OUT_FIG))
        if "wide_dw" not in nul:
            v = (dsum * times) @ wx
            R["wide_dw"] = (v, capped(sum_bound(a_dsum @ np.abs(wx), n_w, cd + 1), dsum @ wx, SUM_FIG))
        if "wide_dbias" not in nul and c["wide_bias"]:
            v = np.array([np.sum(dsum * times)])
            R["wide_dbias"] = (v, capped(sum_bound(a_dsum.sum(), n_w, cd), dsum.sum(), SUM_FIG))
    R["chained"] = dict(dzh2=dz2w, dzh1=dz1w)
    return R


def applies(defect, c):
    masked = bool(c["relu"]) or c["p"] > 0
    return {"stats_drop_last_row": True, "biased_running_var": c["running"], "drop2_from_seed1": c["p"] > 0,
            "drop_stream_tower0": c["p"] > 0 and c["n_tower"] > 1, "seed_offset_ignored": c["p"] > 0 and c["step"] is not None,
            "mask_from_z": masked, "no_mask_scale": c["p"] > 0, "block_M": c["M"] > ROWS,
            "loss_all_towers": bce(c) and c["n_tower"] > 1, "group_unclamped": bce(c) and c["group"] == "outside",
            "wide_two_towers": c["wide"] > 0 and ("wide_dw" not in c["null"] or ("wide_dx" not in c["null"] and c["acc_wide"])),
            "wide_no_tower": c["wide"] > 0 and not {"wide_dw", "wide_dx"} <= set(c["null"]),
            "acc_dx_off": any(c["acc_dx"]) and "dx" not in c["null"], "acc_wide_off": c["wide"] > 0 and c["acc_wide"] and "wide_dx" not in c["null"],
            "no_bo": c["bo"], "operand_unrounded": True}[defect]


# ------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------
def compare(got, want, what):
    """got: name -> array; want: name -> (float64, bound).  The one comparator of the CPU and the GPU tests."""
    from helpers import assert_bounded
    for k, v in want.items():
        if isinstance(v, tuple):
            assert k in got, f"{what}: {k} not produced"
            assert_bounded(got[k], v[0], v[1], f"{what} {k}")
        elif k.startswith("nbt"):
            assert k in got and int(got[k]) == int(v), f"{what}: {k} is {got.get(k)}, expected {v}"


def rounded(R):
    """a float64 result as a device would store it: fp32, the bf16 tensors rounded to bf16"""
    out = {}
    for k, v in R.items():
        if isinstance(v, tuple):
            a = v[0].astype(np.float32)
            out[k] = B.bf16_round(a) if k.startswith(("a1h_", "dzh")) else a
        elif k.startswith("nbt"):
            out[k] = v
    return out


def saved(got, c):
    """the S of ref_forward / ref_backward from a flat result"""
    n = c["n_tower"]
    S = {k: [got[f"{k}_{t}"] for t in range(n)] for k in ("z1", "a1h", "z2", "a2", "mean1", "inv1", "mean2", "inv2", "dzh2", "dzh1")
         if f"{k}_0" in got}
    S["out"] = got["out"]
    return S


# ------------------------------------------------------------------------------------------------------------------------
# the launches in fp32 / bf16 numpy, in the kernels' operation order: stands in for a device on the CPU
# ------------------------------------------------------------------------------------------------------------------------
def kernel32(c, D):
    M, n, K, H0 = c["M"], c["n_tower"], c["wide"], c["H0"]
    one = np.float32(1)
    got = {}
    Z1 = [f32(f32(D["x"][t]) @ f32(D["W1"][t]).T) + f32(D["b1"][t]) for t in range(n)]
    f1 = B.kernel_forward32(bn_spec(c, 1), bn_data(c, D, 1, Z1))
    A1 = [f1[t]["yh"] for t in range(n)]
    Z2 = [f32(f32(A1[t]) @ f32(D["W2"][t]).T) + f32(D["b2"][t]) for t in range(n)]
    f2 = B.kernel_forward32(bn_spec(c, 2), bn_data(c, D, 2, Z2))
    A2 = [f2[t]["y"] for t in range(n)]
    wide = np.zeros(M, np.float32)
    if K:
        wide = f32(f32(D["wx"]) @ f32(D["ww"]))
        if D["wb"] is not None:
            wide = wide + D["wb"][0]
    out = np.zeros((M, n), np.float32)
    for t in range(n):
        acc = f32(A2[t] @ f32(D["wo"][t]))
        if D["bo"][t] is not None:
            acc = acc + D["bo"][t][0]
        if K:
            acc = acc + wide
        if c["sigmoid"]:
            with np.errstate(over="ignore"):
                acc = one / (one + np.exp(-acc))
        out[:, t] = acc
        for l, f, Z in ((1, f1, Z1), (2, f2, Z2)):
            got[f"z{l}_{t}"], got[f"mean{l}_{t}"], got[f"inv{l}_{t}"] = Z[t], f[t]["save_mean"], f[t]["save_invstd"]
            if c["running"]:
                got[f"rm{l}_{t}"], got[f"rv{l}_{t}"] = f[t]["running_mean"], f[t]["running_var"]
            if c["nbt"]:
                got[f"nbt{l}_{t}"] = D[f"nbt{l}"][t] + 1
        got[f"a1h_{t}"], got[f"a2_{t}"] = A1[t], A2[t]
    got["out"] = out
    # ---- backward
    nul = set(c["null"])
    if bce(c):
        own, y, inv = own_tower(c, D), f32(D["y"]), np.float32(inv_count(c))
        o = out[np.arange(M), own]
        with np.errstate(divide="ignore"):
            lp = (y - one) * np.maximum(np.log1p(-o), np.float32(-100)) - y * np.maximum(np.log(o), np.float32(-100))
        got["loss"] = f32([f64(lp).sum() * float(inv)])
        dout = np.zeros((M, n), np.float32)
        dout[np.arange(M), own] = inv * (o - y) / np.maximum((one - o) * o, np.float32(1e-12))
    else:
        dout = f32(D["dout"])
    d = f32(dout * out * (one - out)) if c["sigmoid"] else dout
    dy2 = [f32(d[:, t:t + 1] * f32(D["wo"][t])[None, :]) for t in range(n)]
    g2 = B.kernel_backward32(bn_spec(c, 2), bn_data(c, D, 2, Z2, dy=dy2), A2, [f2[t]["save_mean"] for t in range(n)],
                             [f2[t]["save_invstd"] for t in range(n)])
    dy1 = [f32(f32(g2[t]["dxh"]) @ f32(D["W2"][t])) for t in range(n)]
    g1 = B.kernel_backward32(bn_spec(c, 1), bn_data(c, D, 1, Z1, dy=dy1), A1, [f1[t]["save_mean"] for t in range(n)],
                             [f1[t]["save_invstd"] for t in range(n)])
    for t in range(n):
        if "dwo" not in nul:
            got[f"dwo_{t}"] = f32(f64(f32(d[:, t:t + 1] * A2[t])).sum(0))
        if "dbo" not in nul and c["bo"]:
            got[f"dbo_{t}"] = f32([f64(d[:, t]).sum()])
        for l, g in ((2, g2), (1, g1)):
            got[f"dzh{l}_{t}"] = g[t]["dxh"]
            if "dgamma" not in nul:
                got[f"dgamma{l}_{t}"] = g[t]["dgamma"]
            if "dbeta" not in nul:
                got[f"dbeta{l}_{t}"] = g[t]["dbeta"]
        if "dx" not in nul:
            v = f32(f32(g1[t]["dxh"]) @ f32(D["W1"][t]))
            got[f"dx_{t}"] = f32(D["dx0"][t] + v) if c["acc_dx"][t] else v
    if K:
        dsum = np.zeros(M, np.float32)
        for t in range(n):
            dsum = dsum + d[:, t]
        if "wide_dx" not in nul:
            v = f32(dsum[:, None] * f32(D["ww"])[None, :])
            got["wide_dx"] = f32(D["wdx0"] + v) if c["acc_wide"] else v
        if "wide_dw" not in nul:
            got["wide_dw"] = f32(f32(dsum[:, None] * f32(D["wx"])).sum(0, dtype=np.float32))
        if "wide_dbias" not in nul and c["wide_bias"]:
            got["wide_dbias"] = f32([dsum.sum(dtype=np.float32)])
    return got
