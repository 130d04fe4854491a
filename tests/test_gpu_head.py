"""The tower head (csrc/head.hip: cdc_head_fwd, cdc_head_bwd, cdc_head_workspace_floats) straight through the C-ABI against a
float64 restatement of the formulas of include/cdcmdr.h — every stride, flag and NULL pointer chosen by the test.

Buffers are padded (helpers.PadBuf): input padding is NaN, output padding a sentinel that must come back bit-unchanged;
accumulate targets start from random values, plain stores from NaN.  Bounds are derived (helpers.sum_bound): a sum of n fp32 terms
may be off by (n + c) 2^-24 sum|term_i|, c counting the formula's further roundings, and never more than the suite's present
figure for that kind of quantity (helpers.capped).  test_head_bounds_reject_seeded_defects shows on the CPU that these bounds
reject seven seeded defects at every shape used here."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import (OUT_FIG, PAD, SUM_FIG, U24, PadBuf, assert_bits_equal, assert_bounded, assert_close, capped, host_ulps, nan_like,
                     sum_bound, ulp32)

gpu = pytest.mark.gpu
PARTS = 256                                     # CDC_ROWDOT_PARTS

# towers (K per tower), wide_K, M, then what the case switches on; dx/dw: towers whose dx resp. dw+dbias pointer is NULL
CASES = {
    "a": dict(K=(33,), wide=None, M=1, n_add=0, bias=False, sigmoid=0, acc_dx=(0,), ld_dout_extra=2),
    "b": dict(K=(1, 33, 64), wide=26, M=7, n_add=1, acc_dx=(1, 0, 1), acc_wide=1, acc_add=(0,), wide_out=True, no_dx=(1,)),
    "c": dict(K=(64, 64, 64, 64), wide=512, M=256, n_add=2, acc_dx=(0, 1, 0, 1), acc_wide=0, acc_add=(1, 0), wide_out=False,
              wide_bias=False, no_dw=(2,)),
    "d": dict(K=(64, 65), wide=26, M=257, n_add=1, acc_dx=(1, 1), acc_wide=1, acc_add=(1,), wide_out=True),
    "e": dict(K=(32, 32, 32), wide=513, M=255, n_add=0, acc_dx=(0, 1, 0), acc_wide=0, wide_out=True, ld_dout_extra=1),
    "f": dict(K=(16, 40, 64, 8, 64), wide=26, M=1000, n_add=2, acc_dx=(1, 0, 1, 0, 1), acc_wide=1, acc_add=(0, 1), wide_out=False,
              no_dw=(3,)),
    "g": dict(K=(128,) * 8, wide=600, M=300, n_add=1, acc_dx=(0, 1) * 4, acc_wide=0, acc_add=(0,), wide_out=True, no_dx=(5,),
              no_dadd=(0,)),
}
BCE_CASES = ("b", "d", "f")


def _spec(name):
    s = dict(bias=True, sigmoid=1, acc_wide=0, acc_add=(), wide_out=False, wide_bias=True, no_dx=(), no_dw=(), no_dadd=(), ld_dout_extra=0)
    s.update(CASES[name])
    s["name"] = name
    return s


def _sig(z):
    e = np.exp(-np.abs(z))                      # float64, relative accuracy kept at either end
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def make_data(s, bce=None):
    """N(0,1) inputs, weights of order 1/sqrt(K).  bce = (label kind, group kind): labels, tower indices and a large addend that
    drives some logits to +-40 (outputs exactly 1 in fp32) and to -110 (exactly 0), so that both clamps of the loss act."""
    rng = np.random.default_rng(sum(map(ord, s["name"])) + (17 if bce else 0))
    M, nt = s["M"], len(s["K"])
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    D = dict(x=[f32(rng.standard_normal((M, K))) for K in s["K"]],
             w=[f32(rng.standard_normal(K) / np.sqrt(K)) for K in s["K"]],
             b=[f32(0.3 * rng.standard_normal(1)) if s["bias"] else None for _ in s["K"]],
             add=[f32(0.5 * rng.standard_normal((M, 1))) for _ in range(s["n_add"])],
             dout=f32(rng.standard_normal((M, nt))),
             dx0=[f32(rng.standard_normal((M, K))) for K in s["K"]],
             dadd0=[f32(rng.standard_normal((M, 1))) for _ in range(s["n_add"])])
    if s["wide"]:
        Kw = s["wide"]
        D.update(wx=f32(rng.standard_normal((M, Kw))), ww=f32(rng.standard_normal(Kw) / np.sqrt(Kw)),
                 wb=f32(0.3 * rng.standard_normal(1)) if s["wide_bias"] else None, wdx0=f32(rng.standard_normal((M, Kw))))
    if bce:
        kind, gkind = bce
        y = rng.integers(0, 2, size=M)
        if kind == "f32":
            y = np.where(rng.random(M) < 0.25, rng.random(M), y)               # soft labels: both terms of the loss at once
        D["y"] = y.astype(np.int16 if kind == "i16" else np.float32)
        g = None if gkind == "none" else rng.integers(0, nt, size=M).astype(np.int64)
        if gkind == "outside":
            g[::5] = -1
            g[2::7] = nt
        D["group"] = g
        big = D["add"][0]                                                        # (every BCE case has an addend)
        for v, rows in ((40.0, slice(0, None, 6)), (-40.0, slice(1, None, 6)), (-110.0, slice(3, None, 11))):
            big[rows] = v
    return D


# ------------------------------------------------------------------------------------------------------------------------
# float64 restatement of include/cdcmdr.h (cdc_head_args) with its error bounds; `defect` seeds one wrong term
# ------------------------------------------------------------------------------------------------------------------------
def ref_forward(s, D, defect=None):
    M, nt = s["M"], len(s["K"])
    d64 = lambda a: np.asarray(a, dtype=np.float64)
    shared, a_shared, n_shared = np.zeros(M), np.zeros(M), 0
    if s["wide"]:
        shared, a_shared = d64(D["wx"]) @ d64(D["ww"]), np.abs(d64(D["wx"])) @ np.abs(d64(D["ww"]))
        n_shared = s["wide"] + 1                                                 # the products, and shared's own rounding
        if D["wb"] is not None:
            shared, a_shared, n_shared = shared + float(D["wb"][0]), a_shared + abs(float(D["wb"][0])), n_shared + 1
    adds = D["add"][:-1] if defect == "no_addend" else D["add"]
    z, dz = np.zeros((M, nt)), np.zeros((M, nt))
    for t, K in enumerate(s["K"]):
        x, w = d64(D["x"][t]), d64(D["w"][t])
        if defect == "swap_w" and t < 2 and nt >= 2:
            k = min(s["K"][0], s["K"][1])
            w = w.copy()
            w[:k] = d64(D["w"][1 - t])[:k]
        if defect == "drop_k" and t == nt - 1:
            x, w = x[:, :K - 1], w[:K - 1]
        acc, a_acc, c = x @ w, np.abs(x) @ np.abs(w), 1
        if D["b"][t] is not None:
            acc, a_acc, c = acc + float(D["b"][t][0]), a_acc + abs(float(D["b"][t][0])), c + 1
        if s["wide"]:
            acc, a_acc, c = acc + shared, a_acc + a_shared, c + 1
        for ad in adds:
            acc, a_acc, c = acc + d64(ad)[:, 0], a_acc + np.abs(d64(ad)[:, 0]), c + 1
        z[:, t], dz[:, t] = acc, sum_bound(a_acc, K + n_shared, c)
    R = {"z": z, "dz": dz}
    if s["wide"] and s["wide_out"]:
        R["wide_out"] = (shared.reshape(M, 1), capped(sum_bound(a_shared, n_shared, 0), shared, OUT_FIG).reshape(M, 1))
    if not s["sigmoid"]:
        R["out"] = (z, capped(dz, z, OUT_FIG))
        return R
    out = _sig(z)
    # 1 / (1 + expf(-z)) in fp32 on the host over these logits against float64: 2.6 ulp of the result at worst (measured on every
    # case of this file, the +-40 / -110 rows included, where the result is exactly 1, 4e-18 or 0); allowed 4x = 10.4 ulp, the
    # device's expf need not match the host's last bits
    z32 = z.astype(np.float32)
    with np.errstate(over="ignore"):
        host = np.float32(1) / (np.float32(1) + np.exp(-z32))
    R["sigmoid_ulps"] = host_ulps(host, _sig(z32.astype(np.float64)))
    SIGMOID_ULPS_HOST = 2.6
    prop = np.maximum(_sig(z + dz) - out, out - _sig(z - dz))                    # the logit's bound carried through the sigmoid
    R["out"] = (out, capped(prop + 4 * SIGMOID_ULPS_HOST * ulp32(out), out, OUT_FIG))
    return R


def ref_backward(s, D, out32, bce=None, defect=None):
    """From the fp32 `out` the kernel reads: every gradient, and with bce the loss, as name -> (want, bound)."""
    M, nt = s["M"], len(s["K"])
    d64 = lambda a: np.asarray(a, dtype=np.float64)
    o = d64(out32)
    R, cd = {}, 0
    if bce:
        y = d64(D["y"])
        own = np.zeros(M, dtype=np.int64) if D["group"] is None else D["group"].copy()
        own[(own < 0) | (own >= nt)] = 0                                         # "clamped into the launch's columns": column 0
        oo = o[np.arange(M), own]
        inv = 1.0 / (M + 1 if defect == "count" else M)
        with np.errstate(divide="ignore"):
            la, lb = np.maximum(np.log1p(-oo), -100.0), np.maximum(np.log(oo), -100.0)
        rows = (y - 1.0) * la - y * lb
        mag = np.abs((y - 1.0) * la) + np.abs(y * lb)
        # (t - 1) max(log1pf(-o), -100) - t max(logf(o), -100) in fp32 on the host against float64, in ulps of the two terms'
        # magnitudes: 2.4 ulp at worst over the cases of this file; allowed 4x = 9.6 ulp per row.  The rows are added in double.
        o32, y32 = oo.astype(np.float32), y.astype(np.float32)
        with np.errstate(divide="ignore"):
            host = (y32 - np.float32(1)) * np.maximum(np.log1p(-o32), np.float32(-100)) - y32 * np.maximum(np.log(o32), np.float32(-100))
        R["loss_ulps"] = max(0.5, float(np.max(np.abs(host.astype(np.float64) - rows) / ulp32(mag))))
        LOSS_ULPS_HOST = 2.4
        loss = rows.sum() * inv
        R["loss"] = (np.array([loss]), capped(np.array([inv * np.sum(4 * LOSS_ULPS_HOST * ulp32(mag)) + 2 * U24 * abs(loss)]), loss, OUT_FIG))
        dout = np.zeros((M, nt))
        dout[np.arange(M), own] = inv * (oo - y) / np.maximum((1.0 - oo) * oo, 1e-12)
        cd = 7                                                                   # o - t, 1 - o, their product, 1e-12f, the quotient, inv (twice: 1/M)
    else:
        dout = d64(D["dout"])
    d = dout * o * (1.0 - o) if s["sigmoid"] else dout
    cd += 3 if s["sigmoid"] else 0
    ad = np.abs(d)
    dsum, a_dsum = d.sum(1), ad.sum(1)
    per = -(-M // PARTS)
    keep = np.ones(M)
    if defect == "drop_row":
        keep[min(3 * per, M) - 1] = 0.0                                          # the last row of part 2 (not one of the saturated rows)
    for t, K in enumerate(s["K"]):
        x, w = d64(D["x"][t]), d64(D["w"][t])
        if t not in s["no_dx"]:
            v = d[:, t:t + 1] * w[None, :]
            b = (cd + 1) * U24 * np.abs(v)
            if s["acc_dx"][t] and defect != "acc_off":
                v = d64(D["dx0"][t]) + v
                b = b + U24 * np.abs(v)
            R[f"dx{t}"] = (v, capped(b, v, OUT_FIG))
        if t not in s["no_dw"]:
            R[f"dw{t}"] = (((d[:, t] * keep) @ x).reshape(1, K), capped(sum_bound(ad[:, t] @ np.abs(x), M, cd + 1), d[:, t] @ x, SUM_FIG).reshape(1, K))
            R[f"dbias{t}"] = (np.array([[np.sum(d[:, t] * keep)]]), capped(sum_bound(ad[:, t].sum(), M, cd), d[:, t].sum(), SUM_FIG).reshape(1, 1))
    for i in range(s["n_add"]):
        if i in s["no_dadd"]:
            continue
        v, b = dsum.copy(), sum_bound(a_dsum, nt, cd)
        if s["acc_add"][i]:
            v = d64(D["dadd0"][i])[:, 0] + v
            b = b + U24 * np.abs(v)
        R[f"d_addend{i}"] = (v.reshape(M, 1), capped(b, v, OUT_FIG).reshape(M, 1))
    if s["wide"]:
        wx, ww, Kw = d64(D["wx"]), d64(D["ww"]), s["wide"]
        src = d[:, 0] if defect == "wide_from_tower0" else dsum
        v = src[:, None] * ww[None, :]
        b = sum_bound(a_dsum[:, None] * np.abs(ww)[None, :], nt, cd + 1)
        if s["acc_wide"]:
            v = d64(D["wdx0"]) + v
            b = b + U24 * np.abs(v)
        R["wide_dx"] = (v, capped(b, v, OUT_FIG))
        R["wide_dw"] = (((src * keep) @ wx).reshape(1, Kw), capped(sum_bound(a_dsum @ np.abs(wx), M + nt, cd + 1), dsum @ wx, SUM_FIG).reshape(1, Kw))
        if D["wb"] is not None:
            R["wide_dbias"] = (np.array([[np.sum(src * keep)]]), capped(sum_bound(a_dsum.sum(), M + nt, cd), dsum.sum(), SUM_FIG).reshape(1, 1))
    return R


def compare(got, want, what):
    """got: name -> fp32 array; want: name -> (float64, bound).  The one comparator of the CPU and the GPU tests."""
    for k, v in want.items():
        if isinstance(v, tuple):
            assert k in got, f"{what}: {k} not produced"
            assert_bounded(got[k], v[0], v[1], f"{what} {k}")


# ------------------------------------------------------------------------------------------------------------------------
# the bounds must bite (CPU)
# ------------------------------------------------------------------------------------------------------------------------
FWD_DEFECTS = ("drop_k", "no_addend", "swap_w")
BWD_DEFECTS = ("drop_row", "acc_off", "wide_from_tower0", "count")


def _applies(defect, s, bce):
    return {"drop_k": True, "no_addend": s["n_add"] > 0, "swap_w": len(s["K"]) >= 2, "drop_row": True,
            "acc_off": any(s["acc_dx"][t] for t in range(len(s["K"])) if t not in s["no_dx"]),
            "wide_from_tower0": bool(s["wide"]) and len(s["K"]) >= 2 and not bce, "count": bool(bce)}[defect]


def _rounded(R):
    return {k: v[0].astype(np.float32) for k, v in R.items() if isinstance(v, tuple)}


def test_head_bounds_reject_seeded_defects(monkeypatch):
    """Every derived bound accepts the float64 result rounded to fp32 and rejects it with one defect seeded: the last column of a
    dot product dropped, the last row of a part dropped from the cross-row sums, an addend omitted, two towers' weights swapped,
    accumulate ignored, the wide term's gradient taken from tower 0 alone, and the loss's 1/count off by one row.  Also: no
    bound is looser than the suite's present figures (1e-5 / 1e-6 for outputs, 1e-4 / 1e-5 for cross-row sums), and the
    transcendental allowances written into ref_forward / ref_backward are at least what the host measures here."""
    monkeypatch.delenv("CDC_RECORD_MARGINS", raising=False)                     # (seeded defects are no margins)
    seen = set()
    for name in CASES:
        s = _spec(name)
        for bce in [None] + ([("i16", "none"), ("f32", "valid"), ("i16", "outside")] if name in BCE_CASES else []):
            D = make_data(s, bce)
            F = ref_forward(s, D)
            out32 = F["out"][0].astype(np.float32)
            B = ref_backward(s, D, out32, bce)
            compare(_rounded(F), F, f"{name} clean")
            compare(_rounded(B), B, f"{name} clean")
            if s["sigmoid"]:
                assert F["sigmoid_ulps"] <= 2.6, F["sigmoid_ulps"]
            if bce:
                assert B["loss_ulps"] <= 2.4, B["loss_ulps"]
                assert (out32 == 1).any() and (out32 == 0).any()                 # both clamps act
            for k, (want, bound) in [(k, v) for k, v in list(F.items()) + list(B.items()) if isinstance(v, tuple)]:
                fig = SUM_FIG if k.startswith(("dw", "dbias", "wide_dw", "wide_dbias")) else OUT_FIG
                assert (bound <= fig[1] + fig[0] * np.abs(want) * (1 + 1e-12)).all(), f"{name} {k}: looser than the suite's figure"
            for defect in FWD_DEFECTS + BWD_DEFECTS:
                if not _applies(defect, s, bce):
                    continue
                seen.add(defect)
                if defect in FWD_DEFECTS:
                    got, want = _rounded(ref_forward(s, D, defect)), F
                else:
                    got, want = _rounded(ref_backward(s, D, out32, bce, defect)), B
                with pytest.raises(AssertionError):
                    compare(got, want, f"{name} {defect}")
    assert seen == set(FWD_DEFECTS + BWD_DEFECTS)


# ------------------------------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Launch:
    """One set of fresh padded device buffers for a case and the cdc_head_args over them."""

    def __init__(self, dev, s, D, out32=None, bce=None):
        from cdcmdr_amd import _lib as L
        self.L, self.lib, self.s = L, L.load(), s
        M, nt = s["M"], len(s["K"])
        a = self.a = L.HeadArgs()
        self.keep = []
        inp = lambda v: self._k(PadBuf(dev, v))
        outp = lambda v: self._k(PadBuf(dev, v, out=True))
        a.n_tower, a.sigmoid, a.n_addend, a.M = nt, s["sigmoid"], s["n_add"], M
        self.out = outp(nan_like(M, nt) if out32 is None else out32)
        a.out, a.ld_out = self.out.ptr, self.out.ld
        self.res = {}
        for t, K in enumerate(s["K"]):
            T = a.t[t]
            x, w = inp(D["x"][t]), inp(D["w"][t])
            T.x, T.ldx, T.w, T.K = x.ptr, x.ld, w.ptr, K
            if D["b"][t] is not None:
                T.bias = inp(D["b"][t]).ptr
            T.accumulate_dx = s["acc_dx"][t]
            if t not in s["no_dx"]:
                self.res[f"dx{t}"] = dx = outp(D["dx0"][t] if s["acc_dx"][t] else nan_like(M, K))
                T.dx, T.lddx = dx.ptr, dx.ld
            if t not in s["no_dw"]:
                self.res[f"dw{t}"], self.res[f"dbias{t}"] = outp(nan_like(1, K)), outp(nan_like(1, 1))
                T.dw, T.dbias = self.res[f"dw{t}"].ptr, self.res[f"dbias{t}"].ptr
        if s["wide"]:
            Kw = s["wide"]
            wx, ww = inp(D["wx"]), inp(D["ww"])
            a.wide_x, a.ld_wide, a.wide_w, a.wide_K = wx.ptr, wx.ld, ww.ptr, Kw
            if D["wb"] is not None:
                a.wide_bias = inp(D["wb"]).ptr
                self.res["wide_dbias"] = outp(nan_like(1, 1))
                a.wide_dbias = self.res["wide_dbias"].ptr
            if s["wide_out"]:
                self.wide_out = outp(nan_like(M, 1))
                a.wide_out, a.ld_wide_out = self.wide_out.ptr, self.wide_out.ld
            a.accumulate_wide_dx = s["acc_wide"]
            self.res["wide_dx"] = outp(D["wdx0"] if s["acc_wide"] else nan_like(M, Kw))
            a.wide_dx, a.ld_wide_dx = self.res["wide_dx"].ptr, self.res["wide_dx"].ld
            self.res["wide_dw"] = outp(nan_like(1, Kw))
            a.wide_dw = self.res["wide_dw"].ptr
        for i in range(s["n_add"]):
            ad = inp(D["add"][i])
            a.addend[i], a.ld_addend[i] = ad.ptr, ad.ld
            if i not in s["no_dadd"]:
                a.accumulate_d_addend[i] = s["acc_add"][i]
                self.res[f"d_addend{i}"] = g = outp(D["dadd0"][i] if s["acc_add"][i] else nan_like(M, 1))
                a.d_addend[i], a.ld_d_addend[i] = g.ptr, g.ld
        self.bce = bce
        if bce:
            y = self._k(torch.from_numpy(D["y"]).to(dev))
            if D["y"].dtype == np.int16:
                a.bce_y_i16 = y.data_ptr()
            else:
                a.bce_y_f32 = y.data_ptr()
            if D["group"] is not None:
                a.bce_group = self._k(torch.from_numpy(D["group"]).to(dev)).data_ptr()
            self.loss = self._k(torch.full((1,), float("nan"), device=dev))
            a.bce_loss = self.loss.data_ptr()
            a.bce_partial = self._k(torch.full((PARTS,), float("nan"), dtype=torch.float64, device=dev)).data_ptr()
            a.bce_inv_count = 1.0 / M
        else:
            dout = PadBuf(dev, D["dout"], pad=s["ld_dout_extra"])
            self._k(dout)
            a.d_out, a.ld_dout = dout.ptr, dout.ld
        n_ws = self.lib.cdc_head_workspace_floats(C.byref(a))
        assert n_ws == PARTS * (sum(K + 1 for K in s["K"]) + (s["wide"] + 1 if s["wide"] else 0))
        a.workspace = self._k(torch.full((n_ws,), float("nan"), device=dev)).data_ptr()

    def _k(self, b):
        self.keep.append(b)
        return b

    def forward(self):
        self.L.check(self.lib.cdc_head_fwd(C.byref(self.a), _stream()), "cdc_head_fwd")
        got = {"out": self.out.read("out")}
        if self.s["wide"] and self.s["wide_out"]:
            got["wide_out"] = self.wide_out.read("wide_out")
        return got

    def backward(self):
        self.L.check(self.lib.cdc_head_bwd(C.byref(self.a), _stream()), "cdc_head_bwd")
        got = {k: b.read(k) for k, b in self.res.items()}
        if self.bce:
            got["loss"] = self.loss.cpu().numpy()
        return got


def _covered():
    """What the seven cases switch on, checked once on the CPU side of the GPU tests."""
    S = [_spec(n) for n in CASES]
    assert {s["n_add"] for s in S} == {0, 1, 2}
    assert {v for s in S for t, v in enumerate(s["acc_dx"]) if t not in s["no_dx"]} == {0, 1}
    assert {s["acc_wide"] for s in S if s["wide"]} == {0, 1} and {v for s in S for v in s["acc_add"]} == {0, 1}
    assert any(s["no_dx"] for s in S) and any(s["no_dw"] for s in S) and any(s["no_dadd"] for s in S)
    assert {s["wide_out"] for s in S if s["wide"]} == {False, True} and any(s["wide"] and not s["wide_bias"] for s in S)
    assert any(s["ld_dout_extra"] > 0 for s in S) and any(not s["sigmoid"] and not s["bias"] for s in S)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_head_against_float64(cuda, name):
    """Forward, then the backward from the kernel's own fp32 `out` (twice on fresh buffers: bit-equal), against float64."""
    _covered()
    s = _spec(name)
    D = make_data(s)
    got = Launch(cuda, s, D).forward()
    compare(got, ref_forward(s, D), f"head {name} fwd")
    want = ref_backward(s, D, got["out"])
    g1 = Launch(cuda, s, D, out32=got["out"]).backward()
    g2 = Launch(cuda, s, D, out32=got["out"]).backward()
    for k in g1:
        assert_bits_equal(g1[k], g2[k], f"head {name} {k}: two runs")
    compare(g1, want, f"head {name} bwd")


@gpu
@pytest.mark.parametrize("gkind", ["none", "valid", "outside"])
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("name", BCE_CASES)
def test_head_fused_bce(cuda, name, kind, gkind):
    """The fused BCELoss(mean): loss and gradients against float64 with the header's clamps (log at -100, denominator at 1e-12,
    tower index outside the launch -> column 0), and bit for bit against cdc_bce_fwd_bwd followed by the d_out path."""
    s = _spec(name)
    D = make_data(s, (kind, gkind))
    M, nt = s["M"], len(s["K"])
    fwd = Launch(cuda, s, D).forward()
    compare(fwd, ref_forward(s, D), f"head {name} bce fwd")
    out32 = fwd["out"]
    assert (out32 == 1).any() and (out32 == 0).any()
    want = ref_backward(s, D, out32, (kind, gkind))
    g1 = Launch(cuda, s, D, out32=out32, bce=(kind, gkind)).backward()
    g2 = Launch(cuda, s, D, out32=out32, bce=(kind, gkind)).backward()
    for k in g1:
        assert_bits_equal(g1[k], g2[k], f"head {name} {k}: two runs")
    compare(g1, want, f"head {name} fused bce")
    # the two-launch form: cdc_bce_fwd_bwd on `out`, its dp as d_out of the head's backward
    from cdcmdr_amd import _lib as L
    lib = L.load()
    p, dp = PadBuf(cuda, out32), PadBuf(cuda, nan_like(M, nt), out=True)
    y = torch.from_numpy(D["y"]).to(cuda)
    grp = None if D["group"] is None else torch.from_numpy(D["group"]).to(cuda)
    loss = torch.full((1,), float("nan"), device=cuda)
    L.check(lib.cdc_bce_fwd_bwd(p.ptr, p.ld, None if grp is None else grp.data_ptr(), y.data_ptr() if kind == "i16" else None,
                                y.data_ptr() if kind == "f32" else None, loss.data_ptr(), dp.ptr, dp.ld, M, nt, 1.0 / M, _stream()), "bce")
    D2 = dict(D, dout=dp.read("dp"))
    s2 = dict(s, ld_dout_extra=PAD)
    g3 = Launch(cuda, s2, D2, out32=out32).backward()
    assert_bits_equal(g1["loss"], loss.cpu().numpy(), f"head {name}: fused loss vs cdc_bce_fwd_bwd")
    for k in g3:
        assert_bits_equal(g1[k], g3[k], f"head {name} {k}: fused vs cdc_bce_fwd_bwd + d_out")


@gpu
@pytest.mark.parametrize("name", ["b", "g"])
def test_head_shared_input_gradient_is_rejected(cuda, name):
    """One buffer as the input of two towers, both accumulating into its one gradient: the backward loads a row's gradients before
    it stores any (the all-loads-first body), so the second tower's store would drop the first one's term.  The kernel cannot
    support that; cdc_head_bwd refuses it (in both bodies, so that the answer does not depend on K), plan.TowerHead refuses to
    describe it, and column slices of one buffer side by side — what the models build — still pass."""
    from cdcmdr_amd import _lib as L
    s = dict(_spec(name), acc_dx=(1,) * len(CASES[name]["K"]), no_dx=())
    K = s["K"]
    s["K"] = (K[-1],) + tuple(K[1:])                                             # towers 0 and last: same width
    D = make_data(s)
    out32 = Launch(cuda, s, D).forward()["out"]
    la = Launch(cuda, s, D, out32=out32)
    last = len(s["K"]) - 1
    la.a.t[last].x, la.a.t[last].ldx = la.a.t[0].x, la.a.t[0].ldx
    la.a.t[last].dx, la.a.t[last].lddx = la.a.t[0].dx, la.a.t[0].lddx
    assert la.lib.cdc_head_bwd(C.byref(la.a), _stream()) == -1
    assert b"share an input gradient" in la.lib.cdc_last_error()
    # side by side in one buffer: tower `last` takes the columns after tower 0's
    both = PadBuf(cuda, np.concatenate([D["dx0"][0], D["dx0"][last]], axis=1), out=True)
    lb = Launch(cuda, s, D, out32=out32)
    lb.a.t[0].dx, lb.a.t[0].lddx = both.ptr, both.ld
    lb.a.t[last].dx, lb.a.t[last].lddx = both.ptr + 4 * s["K"][0], both.ld
    L.check(lb.lib.cdc_head_bwd(C.byref(lb.a), _stream()), "cdc_head_bwd, column slices")
    want = ref_backward(s, D, out32)
    got = both.read("dx side by side")
    assert_bounded(got[:, :s["K"][0]], *want["dx0"], "dx0 in a slice")
    assert_bounded(got[:, s["K"][0]:], *want[f"dx{last}"], "dx last in a slice")


@gpu
def test_tower_head_op_refuses_one_input_twice(cuda):
    from cdcmdr_amd import plan as P
    plan = P.Plan(cuda, 8, precision="f32")
    x, out = plan.new(16), plan.new(2)
    lins = [torch.nn.Linear(16, 1).to(cuda) for _ in range(2)]
    with pytest.raises(RuntimeError, match="one input buffer twice"):
        P.TowerHead(plan, [{"x": x, "w": l.weight, "b": l.bias} for l in lins], out)


@gpu
def test_tower_head_op_against_autograd(cuda):
    """plan.TowerHead (the wiring of _fill and of the accumulate flags): three towers, a wide term and one addend that a RowDot
    produces, against torch autograd in float64."""
    from cdcmdr_amd import plan as P
    B, Ks, Kw = 100, (33, 64, 20), 26
    plan = P.Plan(cuda, B, precision="f32")
    gen = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, K, generator=gen) for K in Ks]
    bufs = []
    for xv in xs:
        b = plan.new(xv.shape[1])
        b.tensor().copy_(xv)
        bufs.append(b)
    wide_in, add_in = plan.new(Kw), plan.new(9)
    xw, xa = torch.randn(B, Kw, generator=gen), torch.randn(B, 9, generator=gen)
    wide_in.tensor().copy_(xw)
    add_in.tensor().copy_(xa)
    lins = [torch.nn.Linear(K, 1).to(cuda) for K in Ks]
    lin_w, lin_a = torch.nn.Linear(Kw, 1).to(cuda), torch.nn.Linear(9, 1).to(cuda)
    addend = P.RowDot(plan, [{"x": add_in, "w": lin_a.weight, "b": lin_a.bias}]).outs[0]
    out = plan.new(3)
    P.TowerHead(plan, [{"x": b, "w": l.weight, "b": l.bias} for b, l in zip(bufs, lins)], out,
                wide={"x": wide_in, "w": lin_w.weight, "b": lin_w.bias}, addends=[addend], sigmoid=True)
    plan.finalize([out])
    plan.forward()
    g = torch.randn(B, 3, generator=gen)
    out.grad.tensor().copy_(g)
    plan.backward()
    leaf = lambda t: t.detach().cpu().double().clone().requires_grad_(True)
    xr, wr, ar = [leaf(x) for x in xs], leaf(xw), leaf(xa)
    pw = {id(l): (leaf(l.weight), leaf(l.bias)) for l in lins + [lin_w, lin_a]}
    lin = lambda l, x: x @ pw[id(l)][0].t() + pw[id(l)][1]
    shared = lin(lin_w, wr) + lin(lin_a, ar)
    y = torch.cat([torch.sigmoid(lin(l, x) + shared) for l, x in zip(lins, xr)], dim=1)
    (y * g.double()).sum().backward()
    assert_close(out.tensor(), y, 1e-5, 1e-6, "TowerHead out")
    for i, l in enumerate(lins):
        assert_close(bufs[i].grad.tensor(), xr[i].grad, 1e-5, 1e-6, f"TowerHead dx{i}")
        assert_close(plan.param_grads[id(l.weight)], pw[id(l)][0].grad, 1e-4, 1e-5, f"TowerHead dw{i}")
        assert_close(plan.param_grads[id(l.bias)], pw[id(l)][1].grad, 1e-4, 1e-5, f"TowerHead db{i}")
    assert_close(wide_in.grad.tensor(), wr.grad, 1e-5, 1e-6, "TowerHead d wide in")
    assert_close(add_in.grad.tensor(), ar.grad, 1e-5, 1e-6, "TowerHead d addend in")
    for l, nm in ((lin_w, "wide"), (lin_a, "addend")):
        assert_close(plan.param_grads[id(l.weight)], pw[id(l)][0].grad, 1e-4, 1e-5, f"TowerHead d {nm} w")
        assert_close(plan.param_grads[id(l.bias)], pw[id(l)][1].grad, 1e-4, 1e-5, f"TowerHead d {nm} b")


@gpu
def test_head_argument_checks(cuda):
    """Nothing is launched: return code and cdc_last_error()."""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    s = _spec("b")
    D = make_data(s)
    BADARG, TOOBIG = -1, -2

    def args(bce=None):
        la = Launch(cuda, s, make_data(s, bce) if bce else D, out32=np.full((s["M"], 3), 0.5, np.float32), bce=bce)
        return la, la.a

    def refused(fn, a, code, text):
        assert fn(C.byref(a), _stream()) == code
        assert text in lib.cdc_last_error(), lib.cdc_last_error()

    for n in (0, 9):
        for fn, nm in ((lib.cdc_head_fwd, b"head_fwd"), (lib.cdc_head_bwd, b"head_bwd")):
            la, a = args()
            a.n_tower = n
            refused(fn, a, BADARG, nm + b": bad argument")
        assert lib.cdc_head_workspace_floats(C.byref(a)) == -1
    for fn, nm in ((lib.cdc_head_fwd, b"head_fwd"), (lib.cdc_head_bwd, b"head_bwd")):
        la, a = args()
        a.n_addend = 3
        refused(fn, a, BADARG, nm + b": bad argument")
    la, a = args()
    a.ld_out = 2
    refused(lib.cdc_head_fwd, a, BADARG, b"head_fwd: bad argument")
    la, a = args()
    a.t[1].ldx = 32
    refused(lib.cdc_head_fwd, a, BADARG, b"head_fwd: tower 1 malformed")
    la, a = args()
    a.wide_w = None
    refused(lib.cdc_head_fwd, a, BADARG, b"head_fwd: wide term malformed")
    la, a = args()
    a.workspace = None
    refused(lib.cdc_head_bwd, a, BADARG, b"head_bwd: bad argument")
    la, a = args()
    a.d_out = None
    refused(lib.cdc_head_bwd, a, BADARG, b"needs the output gradient or the fused loss")
    la, a = args(bce=("i16", "none"))
    a.sigmoid = 0
    refused(lib.cdc_head_bwd, a, BADARG, b"the fused BCE needs sigmoid outputs")
    la, a = args()
    a.t[2].K = 2048                                                              # 2 + 34 + 2049 + 27 columns: over the 64 KB of LDS
    refused(lib.cdc_head_bwd, a, TOOBIG, b"too many weight-gradient columns")
    la, a = args()
    assert lib.cdc_head_workspace_floats(C.byref(a)) == PARTS * (2 + 34 + 65 + 27)
    a.n_tower = 9
    assert lib.cdc_head_workspace_floats(C.byref(a)) == -1
