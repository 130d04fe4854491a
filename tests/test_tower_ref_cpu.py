"""tests/tower_ref.py on the CPU: (a) its float64 stages, chained with nothing rounded, are torch autograd's tower; (b) the fp32 /
bf16 restatement in the kernels' operation order stays inside every bound at every case, no element excluded; (c) every seeded
defect breaks at least one bound at every case in which it can act; (d) the ctypes argument block takes the case list's fields."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ref as B
import glinear_ref as GL
import tower_ref as R
from helpers import OUT_FIG, SUM_FIG

CASES = R.cases()
_CACHE = {}


def standin(c):
    """the case's data, the stand-in's results and the two references from them: computed once, shared, never changed"""
    if c["name"] not in _CACHE:
        D = R.make_data(c)
        got = R.kernel32(c, D)
        S = R.saved(got, c)
        _CACHE[c["name"]] = (D, got, S, R.ref_forward(c, D, S), R.ref_backward(c, D, S))
    return _CACHE[c["name"]]


# ------------------------------------------------------------------------------------------------------------------------
# (a) the composed reference against torch autograd, float64
# ------------------------------------------------------------------------------------------------------------------------
def _torch_tower(c, D):
    t64 = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=g)
    M, n, K = c["M"], c["n_tower"], c["wide"]
    ks = 1.0 / (1.0 - float(np.float32(c["p"]))) if c["p"] > 0 else 1.0
    L = dict(x=[], z1=[], z2=[], g1=[], be1=[], g2=[], be2=[], wo=[], bo=[], rm1=[], rv1=[], rm2=[], rv2=[])
    if K:
        wx, ww = t64(D["wx"], True), t64(D["ww"], True)
        wb = t64(D["wb"], True) if D["wb"] is not None else None
        wide = wx @ ww + (wb[0] if wb is not None else 0.0)
    cols = []
    for t in range(n):
        x = t64(D["x"][t], True)
        h = x
        for l in (1, 2):
            z = h @ t64(D[f"W{l}"][t]).T + t64(D[f"b{l}"][t])
            z.retain_grad()
            g, be, rm, rv = t64(D[f"g{l}"][t], True), t64(D[f"be{l}"][t], True), t64(D[f"rm{l}"][t]), t64(D[f"rv{l}"][t])
            h = torch.nn.functional.batch_norm(z, rm, rv, g, be, training=True, momentum=float(np.float32(R.MOMENTUM)), eps=float(np.float32(R.EPS)))
            if c["relu"]:
                h = torch.relu(h)
            if c["p"] > 0:
                h = h * torch.from_numpy(B.keep_mask(R.bn_spec(c, l), t).astype(np.float64)) * ks
            L[f"z{l}"].append(z); L[f"g{l}"].append(g); L[f"be{l}"].append(be); L[f"rm{l}"].append(rm); L[f"rv{l}"].append(rv)
        wo = t64(D["wo"][t], True)
        bo = t64(D["bo"][t], True) if D["bo"][t] is not None else None
        logit = h @ wo + (bo[0] if bo is not None else 0.0) + (wide if K else 0.0)
        cols.append(torch.sigmoid(logit) if c["sigmoid"] else logit)
        L["x"].append(x); L["wo"].append(wo); L["bo"].append(bo)
    out = torch.stack(cols, 1)
    loss = None
    if R.bce(c):
        own = torch.from_numpy(R.own_tower(c, D))
        loss = torch.nn.functional.binary_cross_entropy(out.gather(1, own[:, None])[:, 0], t64(D["y"]), reduction="sum") * R.inv_count(c)
        loss.backward()
    else:
        out.backward(t64(D["dout"]))
    T = {"out": out.detach().numpy()}
    if loss is not None:
        T["loss"] = np.array([float(loss)])
    g = lambda v: v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    for t in range(n):
        T[f"dx_{t}"] = g(L["x"][t]) + (np.asarray(D["dx0"][t], dtype=np.float64) if c["acc_dx"][t] else 0.0)
        T[f"dwo_{t}"] = g(L["wo"][t])
        if L["bo"][t] is not None:
            T[f"dbo_{t}"] = g(L["bo"][t])
        for l in (1, 2):
            T[f"dzh{l}_{t}"], T[f"dgamma{l}_{t}"], T[f"dbeta{l}_{t}"] = g(L[f"z{l}"][t]), g(L[f"g{l}"][t]), g(L[f"be{l}"][t])
            T[f"rm{l}_{t}"], T[f"rv{l}_{t}"] = L[f"rm{l}"][t].numpy(), L[f"rv{l}"][t].numpy()
    if K:
        T["wide_dx"] = g(wx) + (np.asarray(D["wdx0"], dtype=np.float64) if c["acc_wide"] else 0.0)
        T["wide_dw"] = g(ww)
        if wb is not None:
            T["wide_dbias"] = g(wb)
    return T


# p = 0.5 and p = 0: 1 / (1 - p) is the same number in fp32 (the backward's mask_scale) and in float64
TORCH_CASES = [R.case("t_dout", 129, p=0.5, acc_dx=(1, 0, 1), acc_wide=1), R.case("t_bce", 129, p=0.5, form="i16"),
               R.case("t_f32", 67, p=0.0, form="f32", group="outside"), R.case("t_nogroup", 2, p=0.5, form="i16", group="none"),
               R.case("t_relu0", 65, relu=0, p=0.0, sigmoid=0, wide=0, bo=False), R.case("t_nt1", 130, n_tower=1, p=0.5, H0=128),
               R.case("t_one", 257, n_tower=3, p=0.5, form="i16", group="one", wide_bias=False)]


@pytest.mark.parametrize("c", TORCH_CASES, ids=[c["name"] for c in TORCH_CASES])
def test_the_chained_float64_stages_are_torch_autograd(c):
    D = R.make_data(c)
    F = R.ref_forward(c, D, None)
    Bk = R.ref_backward(c, D, F["chained"], chain=True)
    T = _torch_tower(c, D)
    seen = 0
    for k, want in T.items():
        have = F.get(k, Bk.get(k))
        assert have is not None, k
        a, b = np.asarray(have[0], dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
        err = float(np.max(np.abs(a - b))) if a.size else 0.0
        assert err <= 2e-12 * max(1.0, float(np.max(np.abs(b)))), f"{c['name']} {k}: {err:.3e}"
        seen += 1
    assert seen >= 10 * c["n_tower"]


# ------------------------------------------------------------------------------------------------------------------------
# (b) the stand-in inside every bound, (c) every defect outside one
# ------------------------------------------------------------------------------------------------------------------------
def _fig(k):
    if k.startswith(("z1_", "z2_")):
        return GL.Y_FIG
    if k.startswith("dx_"):
        return GL.G_FIG
    if k.startswith(("dwo", "dbo", "dgamma", "dbeta", "wide_dw", "wide_dbias")):
        return SUM_FIG
    return OUT_FIG


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_fp32_restatement_stays_inside_every_bound(c, monkeypatch):
    monkeypatch.delenv("CDC_RECORD_MARGINS", raising=False)
    D, got, S, F, Bk = standin(c)
    R.compare(got, F, f"{c['name']} forward")
    R.compare(got, Bk, f"{c['name']} backward")
    R.compare(R.rounded(F), F, f"{c['name']} forward, float64 rounded once")
    if c["sigmoid"]:
        assert F["sigmoid_ulps"] <= R.SIGMOID_ULPS_HOST
    if R.bce(c):
        assert Bk["loss_ulps"] <= R.LOSS_ULPS_HOST
    produced = {k for k, v in list(F.items()) + list(Bk.items()) if isinstance(v, tuple) or k.startswith("nbt")}
    assert produced == set(got), produced ^ set(got)
    for k, v in list(F.items()) + list(Bk.items()):
        # a1h, a2, dzh: bn_ref takes the figure at the magnitude of the terms and adds the bf16 half ulp (its docstring)
        if isinstance(v, tuple) and not k.startswith(("a1h_", "a2_", "dzh")):
            fig = _fig(k)
            w = np.atleast_1d(v[0])
            b, ok = np.broadcast_to(v[1], w.shape), np.isfinite(w)
            assert (b[ok] <= (fig[1] + fig[0] * np.abs(w[ok])) * (1 + 1e-12)).all(), f"{c['name']} {k}: looser than the suite's figure"
    if c["name"] == "extreme":
        assert (S["out"][:, 0] == 1).all() and (S["out"][:, 2] == 0).all()                    # both clamps of the loss act
    if c["name"] == "degen":
        assert (S["z1"][0][:, 5] == 0).all() and np.isclose(S["inv1"][0][5], R.EPS ** -0.5, rtol=1e-6)
    if c["name"] == "bce_one":
        for t in (0, 2):
            for k in ("dwo", "dgamma1", "dgamma2", "dbeta1", "dbeta2", "dx", "dzh1", "dzh2"):
                assert not Bk[f"{k}_{t}"][0].any() and Bk[f"{k}_{t}"][1].max() < 1e-37        # exactly zero; the bound: half a bf16 ulp at 0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_seeded_defect_breaks_a_bound(defect, monkeypatch):
    monkeypatch.delenv("CDC_RECORD_MARGINS", raising=False)
    acted = 0
    for c in CASES:
        if not R.applies(defect, c):
            continue
        D, got, S, F, Bk = standin(c)
        fwd = defect in R.FWD_DEFECTS
        bad = R.rounded(R.ref_forward(c, D, S, defect) if fwd else R.ref_backward(c, D, S, defect))
        with pytest.raises(AssertionError):
            R.compare(bad, F if fwd else Bk, f"{c['name']} {defect}")
        if defect == "operand_unrounded":                                # both directions contract rounded operands
            with pytest.raises(AssertionError):
                R.compare(R.rounded(R.ref_backward(c, D, S, defect)), Bk, f"{c['name']} {defect} backward")
        acted += 1
    assert acted >= 2, f"{defect} acted in {acted} cases"


def test_the_case_list_reaches_what_the_kernels_branch_on():
    by = {c["name"]: c for c in CASES}
    assert {c["M"] for c in CASES} >= {2, 63, 64, 65, 127, 128, 129, 193, 257, 4160, 16512, 8192}
    assert {c["n_tower"] for c in CASES} == {1, 2, 3, 4} and {c["H0"] for c in CASES} == {64, 128}
    assert {c["wide"] for c in CASES} >= {0, 4, 28, 256, 260, 512} and {c["p"] for c in CASES} == {0.0, 0.2, 0.5}
    assert {c["form"] for c in CASES} == {"dout", "i16", "f32"} and {c["group"] for c in CASES} == {"rand", "none", "outside", "one"}
    for k in ("relu", "sigmoid", "bo", "running", "nbt", "wide_bias", "acc_wide"):
        assert {bool(c[k]) for c in CASES} == {False, True}, k
    assert {k for c in CASES for k in c["null"]} == set(R.NULLABLE) and {c["step"] for c in CASES} == {None, 5}
    assert any(len(set(c["acc_dx"])) == 2 for c in CASES)
    assert all(c["n_tower"] * -(-c["M"] // R.ROWS) <= 256 for c in CASES) and by["resident256"]["n_tower"] * (8192 // R.ROWS) == 256
    assert -(-by["gather4160"]["M"] // 64) > 4 * 16 and -(-by["gather16512"]["M"] // 64) > 8 * 16 and by["gather16512"]["M"] // R.ROWS + 1 > 128
    g = R.make_data(by["bce_outside"])["group"]
    assert (g == -1).any() and (g == 3).any() and ((g >= 0) & (g < 3)).any()
    y = R.make_data(by["bce_f32"])["y"]
    assert y.dtype == np.float32 and ((y > 0) & (y < 1)).any()


# ------------------------------------------------------------------------------------------------------------------------
# (d) the ctypes argument block
# ------------------------------------------------------------------------------------------------------------------------
def test_the_argument_block_takes_the_case_lists_fields():
    from cdcmdr_amd import _lib as L
    assert C.sizeof(L.TowerLayer) == 18 * 8 and C.sizeof(L.TowerDesc) == 10 * 8 + 2 * C.sizeof(L.TowerLayer) + 7 * 8 == 424
    assert C.sizeof(L.TowerArgs) == 264 + L.TOWER_MAX * C.sizeof(L.TowerDesc) == 1960 and L.TOWER_MAX == 4
    assert L.TowerArgs.t.offset == 264 and L.TowerArgs.exchange.offset == 232 and L.TowerArgs.workspace.offset == 216
    assert L.TowerArgs.seed1.offset == 48 and L.TowerArgs.bce_inv_count.offset == 208 and L.TowerDesc.l2.offset == 40 + 144
    for c in CASES:
        a = R.scalar_args(L.TowerArgs(), c)
        assert (a.n_tower, a.H0, a.H1, a.H2, a.M, a.relu, a.sigmoid, a.wide_K, a.accumulate_wide_dx) == \
               (c["n_tower"], c["H0"], 64, 32, c["M"], c["relu"], c["sigmoid"], c["wide"], c["acc_wide"])
        assert a.drop_p == np.float32(c["p"]) and a.seed1 == R.SEED1 and a.seed2 == R.SEED2 and a.eps == np.float32(R.EPS)
        assert tuple(a.t[t].accumulate_dx for t in range(c["n_tower"])) == c["acc_dx"]
        assert a.bce_inv_count == (np.float32(1) / np.float32(c["M"]) if R.bce(c) else 0)
    for name in ("wh", "ldwh", "wt", "ldwt", "bias", "z", "ldz", "dzh", "lddzh", "gamma", "beta", "running_mean", "running_var",
                 "num_batches_tracked", "save_mean", "save_invstd", "dgamma", "dbeta"):
        assert hasattr(L.TowerLayer, name)
    for name in ("xh", "ldxh", "dx", "lddx", "a1h", "lda1h", "a2", "lda2", "wo", "bo", "dwo", "dbo", "dy2", "lddy2", "dy1", "lddy1"):
        assert hasattr(L.TowerDesc, name)
