"""float64 restatement of what include/cdcmdr.h promises for cdc_bn_fwd_args / cdc_bn_bwd_args, every value with a DERIVED error
bound, the two dropout streams of csrc/common.h in integer arithmetic, an fp32 restatement in the kernels' operation order, and
the seeded defects the bounds have to reject.  No GPU: tests/test_bn_ref_cpu.py holds this file, tests/test_gpu_batchnorm.py
holds the launches to it.

A launch is described by a spec (see `spec`): segments C[i] over row groups, the flags of the argument block, and which buffers
exist.  ref_forward / ref_backward return, per segment, name -> (want, bound) with the group's rows only.

The bounds, from the kernels' arithmetic (csrc/rowops.hip; the library is built with -ffp-contract=off):
  * the statistics are double sums of fp32 values: 16 adds per wave, the wave and chunk combination, the stride loop over the
    chunks — N_DBL = chunks + 24 + ranks roundings of 2^-53 cover either dispatch, the GEMM epilogues' partial sums and the
    data-parallel exchange;
  * save_mean is mu rounded once;
  * var = s2/M - mu^2 in double cancels: N_DBL 2^-53 (s2/M + mu^2) absolute on var, carried through 1/sqrt(var + eps) (further
    double roundings: 4 2^-53) and rounded once;
  * y = ((x - mean) invstd) gamma + beta in fp32: the subtraction sees the mean's rounding and its own,
    U24 (|mu| + |x - mu|), scaled by invstd |gamma|; then two products, invstd's own error and the final sum;
  * running stats: 1 - momentum, two products and a sum in fp32 on top of the statistic's error;
  * dz = dy mask_scale is one rounding; xhat = (x - mean) invstd two; dbeta / dgamma are double sums of these rounded once;
    dx = (gamma invstd) (dz - (1/M) (dbeta + xhat dgamma)) takes each operation's rounding in turn;
  * outputs are capped by OUT_FIG, cross-row sums by SUM_FIG (helpers.capped): nothing is looser than the suite's figures.
    For y and dx the figure is taken at the magnitude of the TERMS the fp32 expression combines (capped_terms), as sum_bound
    takes sum |term_i|: invstd |gamma| (|mu| + |x - mu|) + |beta| for y, |gamma| invstd (|dz| + (|dbeta| + |xhat dgamma|) / M)
    for dx.  On |y| alone the figure cannot be met by ANY fp32 evaluation of an ill-conditioned column: two rows with nearly
    equal values have invstd up to eps^-1/2 = 316, the mean's half ulp alone then moves y by U24 |mu| invstd (the fp32
    restatement below, geo64 at M = 2: off by 1.18e-5 where OUT_FIG on |y| allows 6.7e-6), and dx of a two-row group is a
    difference of terms of order |gamma| invstd that cancels to ~0.  For a well-conditioned column (invstd |mu| ~ 1, the
    N(0,1) 2 + 1 data at M >= 63) both readings agree to a small factor, and the derived bound is below either;
  * a bf16 output: the fp32 bound plus half a bf16 ulp."""
import numpy as np

from helpers import OUT_FIG, SUM_FIG, U24, assert_bounded, capped, ulp32

U53 = 2.0 ** -53
ROWS_PER_BLOCK = 64
SEED = 0x1234_5678_9ABC_DEF1
f64 = lambda a: np.asarray(a, dtype=np.float64)
f32 = lambda a: np.asarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# bf16 (round to nearest even, as the device's (__bf16) cast)
# ------------------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = np.isnan(np.asarray(a, dtype=np.float32))
    return np.where(nan, 0x7FC0, r & np.uint64(0xFFFF)).astype(np.uint16)


def bf16_from_bits(u16):
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(a):
    return bf16_from_bits(bf16_bits(a)).reshape(np.shape(a))


def bf16_half_ulp(v):
    return 0.5 * 65536.0 * ulp32(v)


# ------------------------------------------------------------------------------------------------------------------------
# the two dropout streams (csrc/common.h): keep masks [rows, C]
# ------------------------------------------------------------------------------------------------------------------------
def _u64(v):
    return np.uint64(v & 0xFFFFFFFFFFFFFFFF)


def keep_mask_uniform(seed, step, seg, rows, C, p):
    """the one-column dispatch (V = 1): cdc_uniform(seed + step 0xD1342543DE82EF95, ((seg + 64) << 56) ^ (row C + c)) >= p keeps."""
    with np.errstate(over="ignore"):
        sd = _u64(seed)
        if step is not None:
            sd = _u64(int(sd) + (step & 0xFFFFFFFF) * 0xD1342543DE82EF95)
        idx = (np.asarray(rows, dtype=np.uint64)[:, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :]) ^ _u64((seg + 64) << 56)
        z = sd + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return ~(u < np.float32(p))


def _hash32(x):
    with np.errstate(over="ignore"):
        x = x.astype(np.uint32)
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846ca68b)
        x = x ^ (x >> np.uint32(16))
    return x


def keep_mask_bits16(seed, step, seg, rows, C, p):
    """the 16-byte dispatch (V = 4): g2_seed32(seed, step, 64 + seg), g2_drop_bits(row, c >> 1), 16 bits per column (even: low half);
    keeps iff the bits >= round(p 65536)."""
    s = ((seed & 0xFFFFFFFF) ^ (((seed >> 32) & 0xFFFFFFFF) * 0x9E3779B1)) & 0xFFFFFFFF
    if step is not None:
        s ^= ((step & 0xFFFFFFFF) * 0x85EBCA77) & 0xFFFFFFFF
    seed32 = int(_hash32(np.array([(s + (64 + seg) * 0xC2B2AE3D) & 0xFFFFFFFF], dtype=np.uint64))[0])
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    r = (np.asarray(rows, dtype=np.uint64) & np.uint64(0xFFFFFFFF))[:, None]
    c = np.arange(C, dtype=np.uint64)[None, :]
    h = _hash32((np.uint64(seed32) + r * np.uint64(0x9E3779B1) + (c >> np.uint64(1)) * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF))
    bits = np.where((c & np.uint64(1)) == 0, h & np.uint32(0xFFFF), h >> np.uint32(16))
    return bits >= thr


# ------------------------------------------------------------------------------------------------------------------------
# launch descriptions
# ------------------------------------------------------------------------------------------------------------------------
def spec(name, C, M, **kw):
    """C: columns per segment.  pad: extra columns of every matrix (3: rows unaligned -> one column per lane; 4 with every
    C % 4 == 0 -> 16-byte lanes), or one value per segment.  groups: row-group sizes (row_offsets) with seg_group[i] the group of
    segment i.  y / dx: which of the fp32 ("f") and bf16 ("h") outputs exist.  step: the device seed offset, None = NULL."""
    C = tuple(C)
    s = dict(name=name, C=C, M=M, pad=3, groups=None, seg_group=(0,) * len(C), training=1, relu=1, skip_le1=0, eps=1e-5, momentum=0.1,
             drop_p=0.0, step=None, seed=SEED, gb=True, running=True, nbt=True, y="f", xh=False, yb=False, dyh=False, dx="f",
             acc=(0,) * len(C), data="normal")
    s.update(kw)
    if np.isscalar(s["pad"]):
        s["pad"] = (s["pad"],) * len(C)
    assert len(s["pad"]) == len(C) == len(s["seg_group"]) == len(s["acc"])
    return s


def family(s):
    """the dispatch and dropout stream the launch must take (one kernel family, k_bn_*<V, LS>): 16-byte lanes ("v4") iff every
    segment has C % 4 == 0 and 16-byte aligned rows, else one column per lane ("one")."""
    return "v4" if all(c % 4 == 0 for c in s["C"]) and all(p % 4 == 0 for p in s["pad"]) else "one"


def seg_rows(s, i):
    if s["groups"] is None:
        return np.arange(s["M"])
    off = np.concatenate([[0], np.cumsum(s["groups"])])
    g = s["seg_group"][i]
    return np.arange(off[g], off[g + 1])


def launch_rows(s):
    return s["M"] if s["groups"] is None else int(sum(s["groups"]))


def mask_scale(s):
    return float(np.float32(1) / (np.float32(1) - np.float32(s["drop_p"]))) if s["drop_p"] > 0 else 1.0


def keep_mask(s, i):
    rows = seg_rows(s, i)
    fn = keep_mask_bits16 if family(s) == "v4" else keep_mask_uniform
    return fn(s["seed"], s["step"], i, rows, s["C"][i], s["drop_p"])


def make_data(s):
    """x = 2 N(0,1) + 1 (data="normal"); "const": column 0 of every segment constant (var = 0); "offset": |mean| / std = 10^3
    (x = 1000 + N(0,1): the cancellation of s2/M - mu^2; the mean's own half ulp costs any fp32 BatchNorm U24 |mu| invstd |gamma|
    on y there, 6e-5)."""
    rng = np.random.default_rng(sum(map(ord, s["name"])) * 1009 + s["M"])
    R = launch_rows(s)
    D = dict(x=[], gamma=[], beta=[], rm=[], rv=[], nbt=[], dy=[], dx0=[])
    for i, C in enumerate(s["C"]):
        x = f32(rng.standard_normal((R, C)) * 2 + 1)
        if s["data"] == "const":
            x[:, 0] = np.float32(3.140625)
        if s["data"] == "offset":
            x = f32(rng.standard_normal((R, C)) + 1000.0)
        dy = f32(rng.standard_normal((R, C)))
        D["x"].append(bf16_round(x) if s["xh"] else x)
        D["dy"].append(bf16_round(dy) if s["dyh"] else dy)
        D["gamma"].append(f32(rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)))
        D["beta"].append(f32(0.3 * rng.standard_normal(C)))
        D["rm"].append(f32(rng.standard_normal(C)))
        D["rv"].append(f32(rng.uniform(0.5, 2.0, C)))
        D["nbt"].append(int(rng.integers(0, 1000)))
        D["dx0"].append(f32(rng.standard_normal((R, C))))
    return D


def capped_terms(bound, want, terms, fig):
    """helpers.capped with the figure taken at max(|want|, terms): see the module docstring"""
    rtol, atol = fig
    return np.minimum(f64(bound), atol + rtol * np.maximum(np.abs(f64(want)), f64(terms)))


def skipped(s, Mg, backward=False):
    return Mg == 1 or (not backward and bool(s["skip_le1"]) and Mg <= 1)


def _chunks(M):
    return -(-M // ROWS_PER_BLOCK)


def one_pass_limit(M):
    """the |mean| / std at which the derived bound of save_invstd passes OUT_FIG for M rows: relative to invstd the cancellation
    term is (chunks + 25) 2^-53 (1 + 2 ratio^2) / 2 (var + eps ~ var), next to the half ulp of the final rounding."""
    n_dbl = _chunks(M) + 25
    return float(np.sqrt(((OUT_FIG[0] - U24) / (0.5 * n_dbl * U53) - 1.0) / 2.0))


def compare(got, want, what):
    """got: per segment name -> array; want: per segment name -> (float64, bound).  The one comparator of the CPU and GPU tests."""
    for i, (g, w) in enumerate(zip(got, want)):
        for k, v in w.items():
            if isinstance(v, tuple) and k != "pre":
                assert k in g, f"{what}: {k}{i} not produced"
                assert_bounded(g[k], v[0], v[1], f"{what} {k}{i}")


# ------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------
FWD_DEFECTS = ("stats_drop_last_row", "drop_tile_tail", "biased_running_var", "launch_M", "neighbour_gamma")
BWD_DEFECTS = ("launch_M", "acc_off", "neighbour_gamma", "mask_from_x", "no_mask_scale", "one_row_rank")


def _tile_tail(s, C):
    """columns of the last, partial column tile (the whole of it when C fills its tiles)"""
    tw = 64
    if family(s) == "v4":
        cmax = max(s["C"])
        tw = 4 << (6 if cmax >= 256 else 5 if cmax >= 128 else 4 if cmax >= 64 else 3)
    return np.arange(((C - 1) // tw) * tw, C)


def ref_forward(s, D, defect=None, n_ranks=1):
    """Per segment: y (and yh), save_mean, save_invstd, running_mean, running_var as name -> (want, bound) over the group's rows,
    "nbt" the expected num_batches_tracked, "written": whether the saved statistics are stored at all."""
    out = []
    eps, mom, p = float(np.float32(s["eps"])), float(np.float32(s["momentum"])), s["drop_p"]
    for i, C in enumerate(s["C"]):
        rows = seg_rows(s, i)
        Mg = len(rows)
        x = f64(D["x"][i])[rows]
        skip = skipped(s, Mg)
        j = (i + 1) % len(s["C"]) if defect == "neighbour_gamma" else i
        gam = f64(np.resize(D["gamma"][j], C)) if s["gb"] else np.ones(C)
        bet = f64(D["beta"][i]) if s["gb"] else np.zeros(C)
        R = {"nbt": D["nbt"][i] + (1 if s["training"] and not skip else 0), "written": bool(s["training"] and not skip)}
        rm, rv = f64(D["rm"][i]), f64(D["rv"][i])
        if skip:
            pre, by, terms = x.copy(), np.zeros_like(x), np.abs(x)
        else:
            if s["training"]:
                xs = x[:-1] if (defect == "stats_drop_last_row" and Mg >= 2) else x
                Md = launch_rows(s) if defect == "launch_M" else len(xs)
                n_dbl = _chunks(Mg) + 24 + n_ranks
                if Mg == 0:
                    mu, var, a2, a1 = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
                elif defect is None:
                    mu = xs.mean(0)
                    var, a2, a1 = ((xs - mu) ** 2).mean(0), (xs * xs).mean(0), np.abs(xs).mean(0)
                else:
                    mu = xs.sum(0) / Md
                    a2, a1 = (xs * xs).sum(0) / Md, np.abs(xs).mean(0)
                    var = np.maximum(a2 - mu * mu, 0.0)
                dmean = 0.5 * ulp32(mu) + n_dbl * U53 * a1
                dvar = n_dbl * U53 * (a2 + mu * mu)                                # the one-pass cancellation term
                inv = 1.0 / np.sqrt(var + eps)
                g = lambda v: 1.0 / np.sqrt(np.maximum(v, 0.0) + eps)
                dinv = np.maximum(np.abs(g(var + dvar) - inv), np.abs(g(var - dvar) - inv)) + 4 * U53 * inv + 0.5 * ulp32(inv)
                if Mg > 0:                                                         # (an empty group's are not defined by the reference)
                    R["save_mean"] = (mu, capped(dmean, mu, OUT_FIG))
                    R["save_invstd"] = (inv, capped(dinv, inv, OUT_FIG))
                else:
                    R["written"] = None
                R["dvar"], R["dinv_raw"] = dvar, dinv
                if s["running"] and Mg > 0:
                    unb = var if (Mg <= 1 or defect == "biased_running_var") else var * (Mg / (Mg - 1.0))
                    dunb = dvar * (Mg / max(Mg - 1.0, 1.0)) + U24 * np.abs(unb)
                    v = (1 - mom) * rm + mom * mu
                    R["running_mean"] = (v, capped(mom * dmean + U24 * (2 * np.abs((1 - mom) * rm) + np.abs(mom * mu) + np.abs(v)), v, OUT_FIG))
                    v = (1 - mom) * rv + mom * unb
                    R["running_var"] = (v, capped(mom * dunb + U24 * (2 * np.abs((1 - mom) * rv) + np.abs(mom * unb) + np.abs(v)), v, OUT_FIG))
            else:
                mu, dmean = rm, np.zeros(C)
                inv = 1.0 / np.sqrt(rv + eps)
                dinv = 3 * U24 * inv                                               # rv + eps, sqrtf, the quotient: fp32
            A = np.abs(x - mu) * inv * np.abs(gam)
            pre = (x - mu) * inv * gam + bet
            by = (np.abs(gam) * inv * dmean + A * (3 * U24 + dinv / inv) + U24 * np.abs(pre)) * (1 + 1e-6)
            terms = np.abs(gam) * inv * (np.abs(mu) + np.abs(x - mu)) + np.abs(bet)
        if "running_mean" not in R and s["running"]:
            R["running_mean"], R["running_var"] = (rm, np.zeros(C)), (rv, np.zeros(C))   # untouched
        y = np.maximum(pre, 0.0) if s["relu"] else pre
        R["pre"] = (y, by)
        if p > 0:
            ks = 1.0 / (1.0 - float(np.float32(p)))
            R["keep"] = keep_mask(s, i)
            y = np.where(R["keep"], y * ks, 0.0)
            by = np.where(R["keep"], by * ks + 3 * U24 * np.abs(y), 0.0)
        if defect == "drop_tile_tail":
            y = y.copy()
            y[:, _tile_tail(s, C)] = np.nan                                        # never stored: the buffer's NaN stays
        by = capped_terms(by, y, terms * (mask_scale(s) if p > 0 else 1.0), OUT_FIG)
        R["terms"] = {"y": terms}
        if "f" in s["y"]:
            R["y"] = (y, by)
        if "h" in s["y"]:
            R["yh"] = (y, by + bf16_half_ulp(np.abs(y) + by))
        out.append(R)
    return out


def kernel_forward32(s, D):
    """The same launch in fp32 numpy in the kernels' operation order (double chunk partials, then fp32): what the bounds must
    accept besides the float64 result rounded once."""
    out = []
    one, eps, mom, p = np.float32(1), np.float32(s["eps"]), np.float32(s["momentum"]), np.float32(s["drop_p"])
    for i, C in enumerate(s["C"]):
        rows = seg_rows(s, i)
        Mg = len(rows)
        x = f32(D["x"][i])[rows]
        skip = skipped(s, Mg)
        gam = f32(D["gamma"][i]) if s["gb"] else np.ones(C, np.float32)
        bet = f32(D["beta"][i]) if s["gb"] else np.zeros(C, np.float32)
        R = {}
        rm, rv = f32(D["rm"][i]), f32(D["rv"][i])
        v = x.copy()
        if not skip:
            if s["training"]:
                s1, s2 = np.zeros(C), np.zeros(C)
                for k in range(_chunks(Mg)):
                    blk = f64(x[k * 64:(k + 1) * 64])
                    s1, s2 = s1 + blk.sum(0), s2 + (blk * blk).sum(0)
                mu = s1 / Mg if Mg else np.zeros(C)
                var = np.maximum(s2 / Mg - mu * mu, 0.0) if Mg else np.zeros(C)
                mean, inv = f32(mu), f32(1.0 / np.sqrt(var + float(eps)))
                R["save_mean"], R["save_invstd"] = mean, inv
                if s["running"] and Mg > 0:
                    unb = f32(var * (Mg / (Mg - 1.0)) if Mg > 1 else var)
                    R["running_mean"] = (one - mom) * rm + mom * mean
                    R["running_var"] = (one - mom) * rv + mom * unb
            else:
                mean, inv = rm, one / np.sqrt(rv + eps)
            v = (x - mean) * inv * gam + bet
        if "running_mean" not in R and s["running"]:
            R["running_mean"], R["running_var"] = rm, rv
        if s["relu"]:
            v = np.maximum(v, np.float32(0))
        if s["drop_p"] > 0:
            v = np.where(keep_mask(s, i), v * (one / (one - p)), np.float32(0))
        v = f32(v)
        if "f" in s["y"]:
            R["y"] = v
        if "h" in s["y"]:
            R["yh"] = bf16_round(v)
        out.append(R)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# backward: from the fp32 (or bf16) operands the kernel reads — x, the sign of y, dy, gamma, save_mean, save_invstd
# ------------------------------------------------------------------------------------------------------------------------
def ref_backward(s, D, Y, MEAN, INV, defect=None, parts=None, ddy=None, divisor=None):
    """Y[i]: the launch's y buffer [rows of the launch, C] (only its sign is used); MEAN[i] / INV[i]: the saved statistics (in
    eval the running mean and rsqrt(running_var + eps), as the header asks of the caller).  parts[i]: the segment's rows split
    over data-parallel ranks (index arrays into the group's rows): dx then uses the sums over all rows, and dgamma_r<k> /
    dbeta_r<k> are rank k's local sums; without parts dgamma / dbeta are the sums over the group.
    ddy[i]: the error the kernel's own dy already carries against D["dy"][i] (a fused launch forms dy itself: tests/tower_ref.py),
    joined to every bound.  divisor[i]: per row, what a seeded defect divides the column sums by instead of the group's rows."""
    out = []
    ms_true = mask_scale(s)
    ms = 1.0 if defect == "no_mask_scale" else ms_true
    masked = bool(s["relu"]) or ms_true != 1.0
    for i, C in enumerate(s["C"]):
        rows = seg_rows(s, i)
        Mg = len(rows)
        x, y, dy = f64(D["x"][i])[rows], f64(Y[i])[rows], f64(D["dy"][i])[rows]
        j = (i + 1) % len(s["C"]) if defect == "neighbour_gamma" else i
        gam = f64(np.resize(D["gamma"][j], C)) if s["gb"] else np.ones(C)
        skip = skipped(s, Mg, backward=True)
        sign = x if defect == "mask_from_x" else y
        dz = np.where(sign > 0, dy * ms, 0.0) if masked else dy
        ddz = U24 * np.abs(dz) if (masked and ms != 1.0) else np.zeros_like(dz)
        if ddy is not None:
            e = f64(ddy[i])[rows]
            ddz = ddz + (np.where(sign > 0, e * abs(ms), 0.0) if masked else e)
        R = {}
        P = [np.arange(Mg)] if parts is None else parts[i]
        names = [("dgamma", "dbeta")] if parts is None else [(f"dgamma_r{k}", f"dbeta_r{k}") for k in range(len(P))]
        if skip:
            dx, edx, terms = dz, ddz, np.abs(dz)
            for (ng, nb) in names:
                R[ng], R[nb] = (np.zeros(C), np.zeros(C)), (np.zeros(C), np.zeros(C))
        else:
            mean, inv = f64(MEAN[i]), f64(INV[i])
            xh = (x - mean) * inv
            dxh = 2 * U24 * np.abs(xh)
            db, dg, bdb, bdg = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
            for (ng, nb), idx in zip(names, P):
                n_dbl = _chunks(len(idx)) + 24
                lb, lg = dz[idx].sum(0), (dz[idx] * xh[idx]).sum(0)
                if defect == "one_row_rank" and len(idx) == 1:
                    lb, lg = np.zeros(C), np.zeros(C)
                eb = ddz[idx].sum(0) + n_dbl * U53 * np.abs(dz[idx]).sum(0)
                eg = (np.abs(dz[idx]) * dxh[idx] + ddz[idx] * np.abs(xh[idx])).sum(0) + n_dbl * U53 * np.abs(dz[idx] * xh[idx]).sum(0)
                R[nb] = (lb, capped(eb + U24 * np.abs(lb), lb, SUM_FIG))
                R[ng] = (lg, capped(eg + U24 * np.abs(lg), lg, SUM_FIG))
                db, dg, bdb, bdg = db + lb, dg + lg, bdb + eb, bdg + eg
            bdb, bdg = bdb + U24 * np.abs(db) + len(P) * U53 * np.abs(db), bdg + U24 * np.abs(dg) + len(P) * U53 * np.abs(dg)
            gi = gam * inv
            if s["training"]:
                Md = launch_rows(s) if defect == "launch_M" else Mg
                if divisor is not None:
                    Md = f64(divisor[i])[rows].reshape(-1, 1)
                pq = xh * dg
                ep = np.abs(xh) * bdg + np.abs(dg) * dxh + U24 * np.abs(pq)
                q = db + pq
                eq = bdb + ep + U24 * np.abs(q)
                r = q / Md
                er = eq / Md + 2 * U24 * np.abs(r)
                t = dz - r
                et = ddz + er + U24 * np.abs(t)
                dx = gi * t
                edx = (np.abs(gi) * et + 2 * U24 * np.abs(dx)) * (1 + 1e-6)
                terms = np.abs(gi) * (np.abs(dz) + (np.abs(db) + np.abs(pq)) / Md)
            else:
                dx = gi * dz
                edx = (np.abs(gi) * ddz + 2 * U24 * np.abs(dx)) * (1 + 1e-6)
                terms = np.abs(dx)
        if s["acc"][i] and defect != "acc_off":
            dx = f64(D["dx0"][i])[rows] + dx
            edx = edx + U24 * np.abs(dx)
            terms = terms + np.abs(f64(D["dx0"][i])[rows])
        edx = capped_terms(edx, dx, terms, OUT_FIG)
        R["terms"] = {"dx": terms}
        if "f" in s["dx"]:
            R["dx"] = (dx, edx)
        if "h" in s["dx"]:
            R["dxh"] = (dx, edx + bf16_half_ulp(np.abs(dx) + edx))
        out.append(R)
    return out


def kernel_backward32(s, D, Y, MEAN, INV):
    out = []
    one, ms = np.float32(1), np.float32(mask_scale(s))
    masked = bool(s["relu"]) or ms != one
    for i, C in enumerate(s["C"]):
        rows = seg_rows(s, i)
        Mg = len(rows)
        x, y, dy = f32(D["x"][i])[rows], f32(Y[i])[rows], f32(D["dy"][i])[rows]
        gam = f32(D["gamma"][i]) if s["gb"] else np.ones(C, np.float32)
        dz = f32(np.where(y > 0, dy * ms, np.float32(0))) if masked else dy
        R = {}
        if skipped(s, Mg, backward=True):
            dx, R["dgamma"], R["dbeta"] = dz, np.zeros(C, np.float32), np.zeros(C, np.float32)
        else:
            mean, inv = f32(MEAN[i]), f32(INV[i])
            xh = f32((x - mean) * inv)
            s1, s2 = np.zeros(C), np.zeros(C)
            for k in range(_chunks(Mg)):
                sl = slice(k * 64, (k + 1) * 64)
                s1, s2 = s1 + f64(dz[sl]).sum(0), s2 + (f64(dz[sl]) * f64(xh[sl])).sum(0)
            db, dg = f32(s1), f32(s2)
            R["dbeta"], R["dgamma"] = db, dg
            if s["training"]:
                invM = one / np.float32(Mg) if Mg else np.float32(0)
                dx = gam * inv * (dz - invM * (db + xh * dg))
            else:
                dx = gam * inv * dz
        dx = f32(dx)
        if s["acc"][i]:
            dx = f32(D["dx0"][i])[rows] + dx
        if "f" in s["dx"]:
            R["dx"] = dx
        if "h" in s["dx"]:
            R["dxh"] = bf16_round(dx)
        out.append(R)
    return out


def eval_saved(s, D):
    """what the caller passes as save_mean / save_invstd in eval: the running mean and rsqrt(running_var + eps) in fp32"""
    eps = np.float32(s["eps"])
    return [f32(m) for m in D["rm"]], [f32(np.float32(1) / np.sqrt(f32(v) + eps)) for v in D["rv"]]


# ------------------------------------------------------------------------------------------------------------------------
# the shapes the GPU tests run (tests/test_gpu_batchnorm.py) and tests/test_bn_ref_cpu.py seeds the defects at
# ------------------------------------------------------------------------------------------------------------------------
ONE_C = (1, 3, 64, 70)
V4_C = (4, 8, 36, 64, 68, 128, 132, 256, 260)
ROWS = (1, 2, 63, 64, 65, 129, 257, 577)
GROUP_SIZES = (65, 0, 130, 1, 64, 2)                       # {0, 1, 2, 64, 65, 130}, shuffled
GROUP_OF_SEG = (3, 0, 5, 2, 1, 4, 2)                       # non-monotonic; segments 3 and 6 share group 2


def geometry_specs():
    S = []
    for pad, Cs in ((3, ONE_C), (4, V4_C)):
        for C in Cs:
            for M in ROWS:
                S.append(spec(f"geo{C}", (C,), M, pad=pad))
    S.append(spec("mixed", (8, 256), 65, pad=4))
    S.append(spec("fallbackC", (8, 6, 16), 65, pad=4))
    S.append(spec("fallbackLd", (8, 12, 16), 65, pad=(4, 3, 4)))
    S.append(spec("maxseg", tuple(4 * (1 + k % 5) + (64 if k == 7 else 0) for k in range(24)), 66, pad=4))
    return S


def group_specs():
    S = []
    for pad, Cs in ((3, (5, 64, 3, 70, 2, 9, 66)), (4, (8, 64, 4, 68, 12, 16, 132))):
        for le1 in (0, 1):
            S.append(spec(f"groups{pad}{le1}", Cs, int(sum(GROUP_SIZES)), pad=pad, groups=GROUP_SIZES, seg_group=GROUP_OF_SEG, skip_le1=le1,
                          acc=(0, 1, 0, 0, 1, 0, 0)))
    return S


def flag_specs():
    """about a dozen launches that together switch every flag of the two argument blocks, in both dispatches"""
    T = [
        dict(C=(6, 70), M=65, pad=3, relu=0),
        dict(C=(8, 68), M=65, pad=4, relu=0, drop_p=0.25, step=None),
        dict(C=(6, 70), M=130, pad=3, drop_p=0.25, step=3, y="fh", dx="fh"),
        dict(C=(8, 68), M=130, pad=4, drop_p=0.25, step=3, y="fh", dx="fh", acc=(1, 0)),
        dict(C=(6, 70), M=130, pad=3, drop_p=0.25, step=70000, relu=0),
        dict(C=(8, 68), M=130, pad=4, drop_p=0.25, step=70000, y="h", yb=True, dx="h"),
        dict(C=(5, 66), M=65, pad=3, training=0, y="h", yb=True, dx="h", dyh=True),
        dict(C=(8, 132), M=65, pad=4, training=0, relu=0, xh=True, acc=(1, 1)),
        dict(C=(7,), M=66, pad=3, gb=False, running=False, nbt=False, xh=True, dyh=True, acc=(1,)),
        dict(C=(12, 256), M=66, pad=4, gb=False, running=False, nbt=False, xh=True, yb=True, y="fh", dyh=True),
        dict(C=(3, 64), M=129, pad=3, data="const"),
        dict(C=(4, 64), M=129, pad=4, data="const", relu=0),
        dict(C=(3, 64), M=129, pad=3, data="offset"),
        dict(C=(4, 64), M=577, pad=4, data="offset"),
        dict(C=(6,), M=1, pad=3, drop_p=0.25, step=1, acc=(1,)),
        dict(C=(8,), M=1, pad=4, skip_le1=1, drop_p=0.25, step=1, y="fh", dx="fh"),
    ]
    S = [spec(f"flags{k}", **t) for k, t in enumerate(T)]
    assert {s["training"] for s in S} == {0, 1} and {s["relu"] for s in S} == {0, 1} and {s["gb"] for s in S} == {False, True}
    assert {s["step"] for s in S if s["drop_p"] > 0} >= {None, 3, 70000} and {s["y"] for s in S} == {"f", "h", "fh"}
    assert {s["dx"] for s in S} == {"f", "h", "fh"} and {a for s in S for a in s["acc"]} == {0, 1}
    for k in ("xh", "yb", "dyh", "running", "nbt"):
        assert {s[k] for s in S} == {False, True}, k
    for fam in ("one", "v4"):
        assert any(family(s) == fam and s["drop_p"] > 0 for s in S) and any(family(s) == fam and s["xh"] for s in S)
    return S


# data-parallel splits: per rank the group sizes of its launch (None: no row_offsets, the launch's M rows); two segments
DP_SPLITS = {
    "64+64": (None, (64, 64)),
    "100+37": (None, (100, 37)),
    "1+5": ((1, 3), (5, 2)),                               # one rank holds ONE row of group 0, the other five
    "0+5": ((0, 4), (5, 3)),
    "1+0": ((1, 2), (0, 3)),                               # group 0 has one row globally: both ranks skip it
}


def dp_specs(name, pad):
    """-> (union spec, [rank specs], parts): the union holds rank 0's rows of a group, then rank 1's"""
    groups, sizes = DP_SPLITS[name]
    C = (6, 70) if pad == 3 else (8, 68)
    if groups is None:
        u = spec(f"dp{name}", C, sum(sizes), pad=pad)
        ranks = [spec(f"dp{name}r{k}", C, m, pad=pad) for k, m in enumerate(sizes)]
        parts = [[np.arange(0, sizes[0]), np.arange(sizes[0], sum(sizes))] for _ in C]
        return u, ranks, parts
    per_rank = (groups, sizes)
    tot = tuple(a + b for a, b in zip(*per_rank))
    kw = dict(pad=pad, seg_group=(0, 1))
    u = spec(f"dp{name}", C, sum(tot), groups=tot, **kw)
    ranks = [spec(f"dp{name}r{k}", C, max(sum(g), 1), groups=g, **kw) for k, g in enumerate(per_rank)]
    parts = [[np.arange(0, per_rank[0][g]), np.arange(per_rank[0][g], tot[g])] for g in (0, 1)]
    return u, ranks, parts


def dp_rank_rows(u, ranks, parts, k, i):
    """rows of the union's buffers that rank k holds for segment i"""
    return seg_rows(u, i)[parts[i][k]]


def all_specs():
    S = geometry_specs() + group_specs() + flag_specs()
    for name in DP_SPLITS:
        for pad in (3, 4):
            S.append(dp_specs(name, pad)[0])
    return S
