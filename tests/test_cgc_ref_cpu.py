"""tests/cgc_ref.py on the CPU: (a) its float64 stages, chained with nothing rounded, are torch autograd's PLE boundary (two softmax
poolings around Linear + ReLU + mask) and torch autograd's gate pooling, forward and all gradients; (b) the fp32 / bf16 restatement in
the kernels' operation order stays inside every bound at every case, no element excluded; (c) every seeded defect breaks at least
one bound at every case in which it can act; (d) the ctypes argument blocks take the case lists' fields."""
import ctypes as C

import numpy as np
import pytest
import torch

import cgc_ref as R
from helpers import SUM_FIG

MID, POOL = R.mid_cases(), R.pool_cases()
CASES = MID + POOL
_CACHE = {}


def refs(c, D, got, defect=None, fwd=True, bwd=True):
    """the two references of a case from a launch's (here: the stand-in's) saved tensors"""
    F = Bk = None
    if c["op"] == "pool":
        if fwd:
            F = R.ref_pool_fwd(c, D, R.saved_fwd(c, got), defect)
        if bwd:
            Bk = R.ref_pool_bwd(c, D, R.pool_bwd_inputs(c, D), defect)
    else:
        if fwd:
            F = R.ref_mid_fwd(c, D, R.saved_fwd(c, got), defect)
        if bwd:
            Bk = R.ref_mid_bwd(c, D, R.bwd_inputs(c, D), R.saved_bwd(c, got), defect)
    return F, Bk


def standin(c):
    """the case's data, the stand-in's results and the two references from them: computed once, shared, never changed"""
    if c["name"] not in _CACHE:
        D = R.make_data(c)
        got = R.kernel32(c, D)
        _CACHE[c["name"]] = (D, got) + refs(c, D, got)
    return _CACHE[c["name"]]


# ------------------------------------------------------------------------------------------------------------------------
# (a) the composed reference against torch autograd, float64
# ------------------------------------------------------------------------------------------------------------------------
t64 = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=g)
grad = lambda v: v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))


def _activation_leaf(x, mask, scale):
    """a leaf z whose relu + scale is the activation x (z.grad is then the masked, scaled gradient the kernels write)"""
    x = np.asarray(x, dtype=np.float64)
    if not mask:
        z = t64(x, True)
        return z, z
    z = t64(np.where(x > 0, x / scale, -1.0), True)
    return z, torch.relu(z) * scale


def _torch_mid(c, D):
    ne1, ng1, ne2, ng2 = c["counts"]
    T, n = c["topo"], c["B"]
    z1, ex1 = _activation_leaf(D["ex1"], c["mask1"], c["scales"][0])
    X1 = ex1.reshape(n, ne1, R.H1)
    lg1 = [t64(l, True) for l in D["logits1"]]
    p1 = [torch.softmax(l, 1) for l in lg1]
    pooled = [(p1[g][:, :, None] * X1[:, T["sel1"][g], :]).sum(1) for g in range(ng1)]
    ks = float(R.keep_scale(c["p"]))
    z2, ex2 = [], []
    for e in range(ne2):
        z = pooled[T["src_e"][e]] @ t64(D["W"][e]).T + (t64(D["b"][e]) if c["bias"] else 0.0)
        z.retain_grad()
        h = torch.relu(z) if c["relu"] else z
        z2.append(z)
        ex2.append(h * torch.from_numpy(R.drop_keep(c, e).astype(np.float64)) * ks)
    X2 = torch.stack(ex2, 1)
    lg2, p2, outs = [], [], []
    for t in range(ng2):
        l = pooled[T["src_g"][t]] @ t64(D["Wg"][t]).T + (t64(D["bg"][t]) if c["bias"] else 0.0)
        l.retain_grad()
        lg2.append(l)
        p2.append(torch.softmax(l, 1))
        outs.append((p2[t][:, :, None] * X2[:, T["sel2"][t], :]).sum(1))
    sum((o * t64(D["dout"][t])).sum() for t, o in enumerate(outs)).backward()
    Tm = {"ex2": X2.detach().numpy().reshape(n, -1), "dz2_h": np.concatenate([grad(z) for z in z2], 1), "dz1_h": grad(z1)}
    for g in range(ng1):
        Tm[f"probs1_{g}"], Tm[f"pooled_h_{g}"], Tm[f"dl1_{g}"] = p1[g].detach().numpy(), pooled[g].detach().numpy(), grad(lg1[g])
    for t in range(ng2):
        Tm[f"probs2_{t}"], Tm[f"out_{t}"], Tm[f"dl2_{t}"] = p2[t].detach().numpy(), outs[t].detach().numpy(), grad(lg2[t])
    return Tm


def _torch_pool(c, D):
    n, H = c["B"], c["H"]
    z, ex = _activation_leaf(D["ex"], c["mask"], float(np.float32(c["scale"])))
    X = ex.reshape(n, c["n_expert"], H)
    lg = [t64(l, True) for l in D["logits"]]
    p = [torch.softmax(l, 1) for l in lg]
    outs = [(p[g][:, :, None] * X[:, sel, :]).sum(1) for g, sel in enumerate(c["sels"])]
    sum((o * t64(D["dout"][g])).sum() for g, o in enumerate(outs)).backward()
    Tm = {"dex": grad(z) + (np.asarray(D["dex0"], dtype=np.float64) if c["acc"] else 0.0)}
    for g in range(len(c["sels"])):
        Tm[f"probs_{g}"], Tm[f"out_{g}"], Tm[f"dl_{g}"] = p[g].detach().numpy(), outs[g].detach().numpy(), grad(lg[g])
    return Tm


# p = 0.5 and p = 0: 1 / (1 - p) is the same number in fp32 (the backward's scale) and in float64
TORCH_CASES = [R.mid("t_ple3", B=5, p=0.5), R.mid("t_tower5", (12, 6, 12, 5), B=3, p=0.5), R.mid("t_steps", (4, 3, 5, 3), "steps", B=3, p=0.5),
               R.mid("t_max", (4, 8, 16, 8), "max", B=2, p=0.0), R.mid("t_one", (1, 1, 1, 1), "one", B=3, p=0.5),
               R.mid("t_sparse", kind="sparse", B=4, p=0.5), R.mid("t_relu0", relu=0, p=0.0, mask1=0, mask2=0, bias=False, B=4),
               R.pool("t_pool", H=12, B=5), R.pool("t_pool_acc", H=64, B=3, acc=1, scale=2.0),
               R.pool("t_pool_nomask", H=4, B=6, mask=0, n_expert=16, sels=[list(range(16)), [15, 0, 7], [7]])]


@pytest.mark.parametrize("c", TORCH_CASES, ids=[c["name"] for c in TORCH_CASES])
def test_the_chained_float64_stages_are_torch_autograd(c):
    D = R.make_data(c)
    if c["op"] == "pool":
        F = R.ref_pool_fwd(c, D)
        Bk = R.ref_pool_bwd(c, D, F["chained"])
        Tm = _torch_pool(c, D)
    else:
        F = R.ref_mid_fwd(c, D)
        Bk = R.ref_mid_bwd(c, D, F["chained"])
        Tm = _torch_mid(c, D)
    assert set(Tm) == {k for k, v in list(F.items()) + list(Bk.items()) if isinstance(v, tuple)}
    for k, want in Tm.items():
        have = F.get(k, Bk.get(k))
        a, b = np.asarray(have[0], dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert a.shape == b.shape, k
        err = float(np.max(np.abs(a - b)))
        assert err <= 2e-12 * max(1.0, float(np.max(np.abs(b)))), f"{c['name']} {k}: {err:.3e}"


# ------------------------------------------------------------------------------------------------------------------------
# (b) the stand-in inside every bound, (c) every defect outside one
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_fp32_restatement_stays_inside_every_bound(c, monkeypatch):
    monkeypatch.delenv("CDC_RECORD_MARGINS", raising=False)
    D, got, F, Bk = standin(c)
    vis = R.visible(c, got)
    R.compare(vis, F, f"{c['name']} forward")
    R.compare(vis, Bk, f"{c['name']} backward")
    R.compare(R.rounded(c, F), F, f"{c['name']} forward, float64 rounded once")
    assert set(R.rounded(c, F)) | set(R.rounded(c, Bk)) == set(vis), set(R.rounded(c, F)) ^ set(vis)
    for k, v in list(F.items()) + list(Bk.items()):
        if isinstance(v, tuple):
            w, b = v[0], np.broadcast_to(v[1], v[0].shape)
            ok = np.isfinite(w)
            assert ok.all() and (b >= 0).all(), k
            assert (b <= (SUM_FIG[1] + SUM_FIG[0] * np.abs(w)) * (1 + 1e-12)).all(), f"{c['name']} {k}: looser than the suite's figure"
    if c["name"].startswith("one_"):                                 # n_sel = 1: probabilities exactly 1, gate-logit gradients exactly 0
        assert (got["probs1_0"] == 1).all() and (got["probs2_0"] == 1).all() and not got["dl1_0"].any() and not got["dl2_0"].any()
        assert (F["probs1_0"][0] == 1).all() and not Bk["dl2_0"][0].any()
    if c["op"] == "mid" and c["p"] > 0:                              # a dropped element: want 0 and bound 0
        assert ((F["ex2"][0] == 0) & (F["ex2"][1] == 0)).mean() > c["p"] / 2
    if c["name"] in ("sparse_b17", "h64"):                           # an expert no gate selects: gradient exactly 0, bound 0
        k, H, e = ("dz2_h", R.H2, 0) if c["op"] == "mid" else ("dex", c["H"], 2)
        assert not Bk[k][0][:, e * H:(e + 1) * H].any() and not Bk[k][1][:, e * H:(e + 1) * H].any()


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_seeded_defect_breaks_a_bound(defect, monkeypatch):
    monkeypatch.delenv("CDC_RECORD_MARGINS", raising=False)
    acted = 0
    fwd = defect in R.FWD_DEFECTS
    for c in CASES:
        if not R.applies(defect, c):
            continue
        D, got, F, Bk = standin(c)
        bad = refs(c, D, got, defect, fwd=fwd, bwd=not fwd)[0 if fwd else 1]
        with pytest.raises(AssertionError):
            R.compare(R.rounded(c, bad), F if fwd else Bk, f"{c['name']} {defect}")
        acted += 1
    assert acted >= 2, f"{defect} acted in {acted} cases"


def test_the_case_lists_reach_what_the_kernels_branch_on():
    by = {c["name"]: c for c in CASES}
    assert {c["counts"] for c in MID} >= {(8, 4, 8, 3), (12, 6, 12, 5), (1, 1, 1, 1), (4, 8, 16, 8)}
    assert {c["B"] for c in MID} >= {1, 15, 16, 17, 35} and {c["p"] for c in MID} == {0.0, 0.2, 0.5} and {c["step"] for c in MID} == {None, R.STEP}
    for k in ("relu", "bias", "mask1", "mask2", "dlh"):
        assert {bool(c[k]) for c in MID} == {False, True}, k
    assert {k for c in MID for k in c["null"]} == {"pooled_h", "out", "out_h"}
    assert any(c["scales"][0] != c["scales"][1] for c in MID) and all(len(set(c["stream_id"])) == c["counts"][2] for c in MID)
    five, mx, st = by["tower5_b17"], by["max_b17"], by["steps_b17"]
    assert five["counts"][1] > 4 and five["counts"][3] > 4                                    # the second gate pass, both levels
    assert five["counts"][2] * 4 + five["counts"][3] == 53 > 48 and five["counts"][1] * 8 == 48 > 32 and five["counts"][0] > 8
    assert [len(R.k_steps(mx, s)) for s in range(8)] == [6, 6, 1, 6, 6, 5, 5, 5]
    assert [[k for k, _, _ in R.k_steps(st, s)] for s in range(3)] == [["e"] * 6, ["e"] * 4 + ["g"] * 2, ["g"]]
    assert {len(s) for s in mx["topo"]["sel2"]} >= {16, 3} and {len(s) for s in mx["topo"]["sel1"]} >= {1, 2, 4}
    sp = by["sparse_b17"]["topo"]["sel2"]
    assert all(1 in s for s in sp) and not any(0 in s for s in sp) and sp[0] == [1, 2, 3, 7]
    assert {c["H"] for c in POOL} == {4, 12, 64, 128, 256, 320} and {c["B"] for c in POOL} >= {1, 5, 67}
    assert {c["n_expert"] for c in POOL} >= {16, 17, 32} and {len(c["sels"]) for c in POOL} >= {1, 16}
    assert {len(s) for c in POOL for s in c["sels"]} >= {1, 16} and {c["acc"] for c in POOL} == {0, 1} == {c["mask"] for c in POOL}
    assert any(c["unaligned"] for c in POOL) and all(c["B"] <= R.ROWS_MAX for c in CASES)
    D = R.make_data(by["ple3_b17"])
    assert (D["ex1"] == 0).mean() > 0.4 and (D["logits1"][0][0] > 9e3).all() and len(set(D["logits1"][0][1])) == 1
    assert D["logits1"][0][2].min() == -80 and D["logits1"][0][2].max() == 80
    a, b = R.make_data(by["ple3_b17"]), R.make_data(by["ple3_b35"])                           # shared data: the first rows agree
    assert np.array_equal(a["ex1"], b["ex1"][:17]) and np.array_equal(a["dout"][2], b["dout"][2][:17])


# ------------------------------------------------------------------------------------------------------------------------
# (d) the ctypes argument blocks
# ------------------------------------------------------------------------------------------------------------------------
def test_the_argument_blocks_take_the_case_lists_fields():
    from cdcmdr_amd import _lib as L
    assert (C.sizeof(L.MidGate1), C.sizeof(L.MidExpert2), C.sizeof(L.MidGate2)) == (112, 32, 136)
    assert C.sizeof(L.CgcMidFwdArgs) == 88 + 8 * 112 + 16 * 32 + 8 * 136 and L.CgcMidFwdArgs.g1.offset == 88
    assert (C.sizeof(L.MidBGate1), C.sizeof(L.MidBExpert2), C.sizeof(L.MidBGate2)) == (112, 24, 144)
    assert C.sizeof(L.CgcMidBwdArgs) == 112 + 8 * 112 + 16 * 24 + 8 * 144 and L.CgcMidBwdArgs.g1.offset == 112
    assert C.sizeof(L.PoolFwdArgs) == 40 + 16 * 128 and C.sizeof(L.PoolBwdArgs) == 88 + 16 * 128
    assert (L.MID_MAX_EXPERT, L.MID_MAX_GATE, L.MAX_SEL, L.MAX_GATES) == (R.MID_MAX_EXPERT, R.MID_MAX_GATE, R.MAX_SEL, R.MAX_GATES)
    lib = L.load()
    for c in MID:
        assert lib.cdc_cgc_mid_fits(*c["counts"]) == 1, c["counts"]  # (4, 8, 16, 8): 153 600 bytes in the backward, exactly the limit
        a, b = R.mid_fwd_args(L.CgcMidFwdArgs(), c), R.mid_bwd_args(L.CgcMidBwdArgs(), c)
        T = c["topo"]
        for x in (a, b):
            assert (x.B, x.H1, x.H2, x.n_exp1, x.n_gate1, x.n_exp2, x.n_gate2) == (c["B"], 128, 64) + c["counts"]
            assert [list(x.g1[g].sel[:x.g1[g].n_sel]) for g in range(x.n_gate1)] == T["sel1"]
            assert [list(x.g2[t].sel[:x.g2[t].n_sel]) for t in range(x.n_gate2)] == T["sel2"]
            assert [x.e2[e].src for e in range(x.n_exp2)] == T["src_e"] and [x.g2[t].src for t in range(x.n_gate2)] == T["src_g"]
        assert (a.relu, a.seed) == (c["relu"], R.SEED) and a.drop_p == np.float32(c["p"])
        assert [a.e2[e].stream_id for e in range(a.n_exp2)] == c["stream_id"]
        assert (b.mask1, b.mask2) == (c["mask1"], c["mask2"]) and (b.scale1, b.scale2) == tuple(np.float32(s) for s in c["scales"])
    for c in POOL:
        for x in (R.pool_args(L.PoolFwdArgs(), c), R.pool_args(L.PoolBwdArgs(), c)):
            assert (x.n_gates, x.n_expert, x.H, x.B) == (len(c["sels"]), c["n_expert"], c["H"], c["B"])
            assert [list(x.gate[g].sel[:x.gate[g].n_sel]) for g in range(x.n_gates)] == c["sels"]
        assert (x.mask_relu, x.accumulate) == (c["mask"], c["acc"]) and x.mask_scale == np.float32(c["scale"])
