"""Multi-tower models at the reference's one-tower-per-domain groupings ("split": 25 towers on Amazon, 50 on Ali-CCP): the wide
gate softmax + pooling kernels against float64, every multi-tower model's forward and gradients at 8 / 25 / 33 / 50 towers
against the oracle, the training step (graph = eager, dense = lazy table), the evaluator at 50 domains, and the launch
sequences of plans within the older limits (unchanged)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import O, assert_close, compare_param_grads, is_pre_bn_bias, make_ids, oracle_grads, sd_cpu

pytestmark = pytest.mark.gpu

F32_RTOL, F32_ATOL = 2e-4, 2e-5          # the fp32 bounds of test_gpu_ple.py: summation order only
# whole models at 25-50 towers: the same summation-order noise, but the gradients of the shared layers sum over every tower and
# the pre-BatchNorm weight gradients of the towers are differences of near-equal sums, so single elements reach ~1e-3 relative
MANY_RTOL, MANY_ATOL = 1e-3, 1e-4
FD = [7, 100, 3, 50, 11, 29]
CFG = types.SimpleNamespace(use_atten=False, use_dcn=False)


# ------------------------------------------------------------------------------------------------------------------------
# wide gate pooling kernels
# ------------------------------------------------------------------------------------------------------------------------
def _table(lib, L, n_expert, sels, cuda):
    n_sel = (C.c_int32 * len(sels))(*[len(s) for s in sels])
    flat = [int(e) for s in sels for e in s]
    sel = (C.c_int32 * len(flat))(*flat)
    n = lib.cdc_gate_pool_wide_table(len(sels), n_expert, n_sel, sel, None, 0)
    assert n > 0
    tab = (C.c_int32 * n)()
    assert lib.cdc_gate_pool_wide_table(len(sels), n_expert, n_sel, sel, tab, n) == n
    return torch.tensor(list(tab), dtype=torch.int32, device=cuda)


def _pool_fwd(cuda, experts, n_expert, H, logits, sels):
    from cdcmdr_amd import _lib as L
    lib = L.load()
    B = experts.shape[0]
    tab = _table(lib, L, n_expert, sels, cuda)
    outs = [torch.full((B, H), float("nan"), device=cuda) for _ in sels]
    probs = [torch.empty((B, len(s)), device=cuda) for s in sels]
    a = L.PoolWideFwdArgs()
    a.n_gates, a.n_expert, a.H, a.B = len(sels), n_expert, H, B
    a.experts, a.ld_exp, a.table = experts.data_ptr(), experts.stride(0), tab.data_ptr()
    for i, s in enumerate(sels):
        G = a.gate[i]
        G.logits, G.ld_logits = logits[i].data_ptr(), logits[i].stride(0)
        G.out, G.ld_out, G.probs, G.out_h, G.n_sel = outs[i].data_ptr(), H, probs[i].data_ptr(), None, len(s)
    L.check(lib.cdc_gate_pool_wide_fwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "wide fwd")
    torch.cuda.synchronize()
    return outs, probs, tab


def _pool_bwd(cuda, experts, n_expert, H, probs, sels, d_outs, tab, d_experts, mask_relu, mask_scale, accumulate):
    from cdcmdr_amd import _lib as L
    lib = L.load()
    B = experts.shape[0]
    d_logits = [torch.full((B, len(s)), float("nan"), device=cuda) for s in sels]
    a = L.PoolWideBwdArgs()
    a.n_gates, a.n_expert, a.H, a.B = len(sels), n_expert, H, B
    a.experts, a.ld_exp, a.table = experts.data_ptr(), experts.stride(0), tab.data_ptr()
    a.d_experts, a.ld_dexp = d_experts.data_ptr(), d_experts.stride(0)
    a.mask_relu, a.mask_scale, a.accumulate, a.d_experts_h = mask_relu, mask_scale, accumulate, None
    for i, s in enumerate(sels):
        G = a.gate[i]
        G.d_out, G.ld_dout, G.probs = d_outs[i].data_ptr(), H, probs[i].data_ptr()
        G.d_logits, G.ld_dlogits, G.d_logits_h, G.n_sel = d_logits[i].data_ptr(), len(s), None, len(s)
    L.check(lib.cdc_gate_pool_wide_bwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "wide bwd")
    torch.cuda.synchronize()
    return d_logits


def _ref64(experts, n_expert, H, logits, sels):
    ex = experts.double().reshape(experts.shape[0], n_expert, H)
    outs, probs = [], []
    for lg, s in zip(logits, sels):
        p = torch.softmax(lg.double(), dim=1)
        probs.append(p)
        outs.append((p.unsqueeze(2) * ex[:, list(s), :]).sum(dim=1))
    return outs, probs


@pytest.mark.parametrize("n_sel", [17, 52, 102, 256])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_wide_gate_pool_forward_against_float64(cuda, n_sel, H):
    B, n_expert = 67, n_sel + 5
    g = torch.Generator().manual_seed(n_sel * 1000 + H)
    experts = torch.randn(B, n_expert * H, generator=g)
    perm = torch.randperm(n_expert, generator=g)
    sels = [perm[:n_sel].tolist(), list(range(n_expert - n_sel, n_expert)), sorted(perm[:n_sel].tolist())]
    logits = [torch.randn(B, n_sel, generator=g) * 3, torch.randn(B, n_sel, generator=g) * 80.0, torch.full((B, n_sel), 7.5)]
    logits[0][5] = 1e4                                        # large logits: the max-subtracted softmax stays finite
    outs, probs, _ = _pool_fwd(cuda, experts.to(cuda), n_expert, H, [t.to(cuda) for t in logits], sels)
    want, wp = _ref64(experts, n_expert, H, logits, sels)
    for i in range(len(sels)):
        assert_close(probs[i], wp[i], 1e-5, 1e-7, f"probs[{i}]")
        assert_close(outs[i], want[i], 1e-5, 2e-6 * float(want[i].abs().max()), f"out[{i}]")
    assert_close(probs[2], torch.full((B, n_sel), 1.0 / n_sel), 1e-6, 0, "equal logits")


@pytest.mark.parametrize("accumulate,mask_relu", [(0, 0), (1, 1), (0, 1)])
def test_wide_gate_pool_backward_against_float64(cuda, accumulate, mask_relu):
    """Several gates select overlapping experts (d_experts is a sum over gates), one expert is selected by no gate, with and
    without accumulate, with the relu mask; two runs are bit-identical."""
    B, H, n_expert = 45, 64, 120
    g = torch.Generator().manual_seed(11 + accumulate + 2 * mask_relu)
    experts = torch.randn(B, n_expert * H, generator=g)
    sels = [list(range(0, 102)), list(range(50, 119)), [3, 7, 60, 100], list(range(118, -1, -2))]
    logits = [torch.randn(B, len(s), generator=g) for s in sels]
    d_outs = [torch.randn(B, H, generator=g) for _ in sels]
    init = torch.randn(B, n_expert * H, generator=g)
    scale = 1.25 if mask_relu else 1.0
    ex_c = experts.to(cuda)
    _, probs, tab = _pool_fwd(cuda, ex_c, n_expert, H, [t.to(cuda) for t in logits], sels)
    runs = []
    for _ in range(2):
        dex = init.clone().to(cuda)
        dl = _pool_bwd(cuda, ex_c, n_expert, H, probs, sels, [t.to(cuda) for t in d_outs], tab, dex, mask_relu, scale, accumulate)
        runs.append((dex.cpu(), [t.cpu() for t in dl]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), "not deterministic"
    # float64 autograd on the same probabilities the kernel saved (as the plan's backward uses them)
    lg64 = [t.double().requires_grad_(True) for t in logits]
    ex64 = experts.double().requires_grad_(True)
    outs, _ = _ref64(ex64, n_expert, H, lg64, sels)
    torch.autograd.backward(outs, [t.double() for t in d_outs])
    want_dex = ex64.grad
    if mask_relu:
        want_dex = torch.where(experts > 0, want_dex * scale, torch.zeros_like(want_dex))
    if accumulate:
        want_dex = want_dex + init.double()
    dex, dl = runs[0]
    assert_close(dex, want_dex, 1e-5, 1e-5, "d_experts")
    assert float(dex.reshape(B, n_expert, H)[:, 119].abs().max()) == (float(init.reshape(B, n_expert, H)[:, 119].abs().max()) if accumulate else 0.0)
    for i in range(len(sels)):
        assert_close(dl[i], lg64[i].grad, 1e-4, 1e-6, f"d_logits[{i}]")


def test_wide_gate_pool_shadows_strides_tail_and_two_launches(cuda):
    """The layouts a plan hands the wide kernels: row strides wider than the rows, H without a multiple of 32 (48), every bf16
    shadow set (out_h, d_logits_h, d_experts_h: the bf16 rounding of the fp32 value written beside it), and 40 gates split
    over two launches of CDC_WIDE_MAX_GATES and 8, the second adding to d_experts."""
    from cdcmdr_amd import _lib as L
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, H, n_expert, n_gate = 37, 48, 90, 40
    g = torch.Generator().manual_seed(77)
    ld_exp = n_expert * H + 16
    experts = torch.randn(B, ld_exp, generator=g)
    sels = [sorted(torch.randperm(n_expert, generator=g)[:int(k)].tolist()) for k in torch.randint(17, 90, (n_gate,), generator=g)]
    logits = [torch.randn(B, len(s) + 3, generator=g) * 2 for s in sels]           # [B, n_sel] views with ld = n_sel + 3
    d_outs = [torch.randn(B, H + 5, generator=g) for _ in sels]                    # [B, H] views with ld = H + 5
    ex_d = experts.to(cuda)
    lg_d = [t.to(cuda) for t in logits]
    do_d = [t.to(cuda) for t in d_outs]
    outs = [torch.full((B, H + 8), float("nan"), device=cuda) for _ in sels]
    outs_h = [torch.zeros((B, H + 8), dtype=torch.bfloat16, device=cuda) for _ in sels]
    probs = [torch.empty((B, len(s)), device=cuda) for s in sels]
    dl = [torch.full((B, len(s) + 2), float("nan"), device=cuda) for s in sels]
    dl_h = [torch.zeros((B, len(s) + 2), dtype=torch.bfloat16, device=cuda) for s in sels]
    dex = torch.full((B, ld_exp), float("nan"), device=cuda)
    dex_h = torch.zeros((B, ld_exp), dtype=torch.bfloat16, device=cuda)
    per = L.WIDE_MAX_GATES
    keep = []
    for c0 in range(0, n_gate, per):
        chunk = list(range(c0, min(n_gate, c0 + per)))
        tab = _table(lib, L, n_expert, [sels[i] for i in chunk], cuda)
        keep.append(tab)
        a = L.PoolWideFwdArgs()
        a.n_gates, a.n_expert, a.H, a.B = len(chunk), n_expert, H, B
        a.experts, a.ld_exp, a.table = ex_d.data_ptr(), ld_exp, tab.data_ptr()
        for k, i in enumerate(chunk):
            G = a.gate[k]
            G.logits, G.ld_logits, G.out, G.ld_out = lg_d[i].data_ptr(), lg_d[i].stride(0), outs[i].data_ptr(), H + 8
            G.probs, G.out_h, G.ld_out_h, G.n_sel = probs[i].data_ptr(), outs_h[i].data_ptr(), H + 8, len(sels[i])
        L.check(lib.cdc_gate_pool_wide_fwd(C.byref(a), st), "wide fwd")
    for t, c0 in enumerate(range(0, n_gate, per)):
        chunk = list(range(c0, min(n_gate, c0 + per)))
        a = L.PoolWideBwdArgs()
        a.n_gates, a.n_expert, a.H, a.B = len(chunk), n_expert, H, B
        a.experts, a.ld_exp, a.table = ex_d.data_ptr(), ld_exp, keep[t].data_ptr()
        a.d_experts, a.ld_dexp, a.d_experts_h, a.ld_dexp_h = dex.data_ptr(), ld_exp, dex_h.data_ptr(), ld_exp
        a.mask_relu, a.mask_scale, a.accumulate = 1, 1.25, 1 if c0 > 0 else 0
        for k, i in enumerate(chunk):
            G = a.gate[k]
            G.d_out, G.ld_dout, G.probs = do_d[i].data_ptr(), H + 5, probs[i].data_ptr()
            G.d_logits, G.ld_dlogits, G.d_logits_h, G.ld_dlogits_h = dl[i].data_ptr(), len(sels[i]) + 2, dl_h[i].data_ptr(), len(sels[i]) + 2
            G.n_sel = len(sels[i])
        L.check(lib.cdc_gate_pool_wide_bwd(C.byref(a), st), "wide bwd")
    torch.cuda.synchronize()
    ex64 = experts[:, :n_expert * H].double().requires_grad_(True)
    lg64 = [t[:, :len(s)].double().requires_grad_(True) for t, s in zip(logits, sels)]
    want, _ = _ref64(ex64, n_expert, H, lg64, sels)
    torch.autograd.backward(want, [t[:, :H].double() for t in d_outs])
    for i, s in enumerate(sels):
        o = outs[i][:, :H].cpu()
        assert_close(o, want[i].detach(), 1e-5, 2e-6 * float(want[i].abs().max()), f"out[{i}]")
        assert torch.equal(outs_h[i][:, :H].cpu(), o.to(torch.bfloat16)), f"out_h[{i}]"
        assert torch.isnan(outs[i][:, H:]).all(), f"out[{i}] written past H"
        d = dl[i][:, :len(s)].cpu()
        assert_close(d, lg64[i].grad, 1e-4, 1e-6, f"d_logits[{i}]")
        assert torch.equal(dl_h[i][:, :len(s)].cpu(), d.to(torch.bfloat16)), f"d_logits_h[{i}]"
        assert torch.isnan(dl[i][:, len(s):]).all(), f"d_logits[{i}] written past n_sel"
    want_dex = torch.where(experts[:, :n_expert * H] > 0, ex64.grad * 1.25, torch.zeros_like(ex64.grad))
    got = dex[:, :n_expert * H].cpu()
    assert_close(got, want_dex, 1e-5, 1e-5, "d_experts over two launches")
    assert torch.equal(dex_h[:, :n_expert * H].cpu(), got.to(torch.bfloat16)), "d_experts_h is the shadow of the sum"
    assert torch.isnan(dex[:, n_expert * H:]).all(), "d_experts written past n_expert * H"


# ------------------------------------------------------------------------------------------------------------------------
# models at many towers (drop-in autograd path, fp32 contractions) against the oracle
# ------------------------------------------------------------------------------------------------------------------------
def _groups(rng, B, n):
    g = rng.integers(0, n, size=B)
    g[: n - 2] = np.arange(n - 2)                             # every domain but the last two present
    g[g == n - 1] = 0                                         # domain n-1 absent (an empty tower in the grouped models)
    g[g == n - 2] = 1
    g[B - 1] = n - 2                                          # domain n-2 has one row
    return g.astype(np.int64)


def _model(name, n, dom_idx, fd):
    from cdcmdr_amd.model.adl import ADL
    from cdcmdr_amd.model.hinet import HiNet
    from cdcmdr_amd.model.mmoe import MMoE
    from cdcmdr_amd.model.pepnet import PEPNet
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.model.star import STAR
    return {
        "ple": lambda: PLE(fd, 4, n, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.0, config=CFG),
        "mmoe": lambda: MMoE(fd, 4, n, 4, (32, 16, 8), (8, 4), dropout=0.0, config=CFG),
        "star": lambda: STAR(fd, 4, n, (16, 8), domain_idx=dom_idx, dropout=0.0, config=CFG),
        "hinet": lambda: HiNet(fd, 4, n_tower=n, sei_dims=(16, 8), tower_dims=(8, 4), domain_idx=dom_idx, device="cuda",
                               dropout=0.0, config=CFG),
        "pepnet": lambda: PEPNet(fd, 4, n, (16, 8), gate_hidden_dim=8, domain_idx=dom_idx, use_ppnet=True, dropout=0.0, config=CFG),
        "epnet": lambda: PEPNet(fd, 4, n, (16, 8), gate_hidden_dim=8, domain_idx=dom_idx, use_ppnet=False, dropout=0.0, config=CFG),
        "adl": lambda: ADL(fd, 4, n_tower=n, tower_dims=(16, 8), domain_idx=dom_idx, dropout=0.0, device="cuda", config=CFG),
    }[name]()


@pytest.mark.parametrize("n", [8, 25, 33, 50])
@pytest.mark.parametrize("name", ["ple", "mmoe", "star", "hinet", "pepnet", "epnet", "adl"])
def test_model_at_many_towers_matches_oracle(cuda, name, n):
    B, dom_idx = 384, 2
    fd = list(FD)
    fd[dom_idx] = n
    torch.manual_seed(n)
    model = _model(name, n, dom_idx, fd).to(cuda).set_precision("f32")
    model.train()
    sd = sd_cpu(model)
    rng = np.random.default_rng(100 + n)
    X = make_ids(rng, B, fd)
    grp = _groups(rng, B, n)
    X[:, dom_idx] = grp
    y = rng.integers(0, 2, size=B).astype(np.float32)
    xg, gg, yg = torch.from_numpy(X).to(cuda), torch.from_numpy(grp).to(cuda), torch.from_numpy(y).to(cuda)
    stats = {}
    if name in ("ple", "mmoe", "pepnet", "epnet"):
        out = model(xg)
        fwd = {"ple": lambda s: O.ple_forward(s, X, fd, n, training=True, stats_out=stats),
               "mmoe": lambda s: O.mmoe_forward(s, X, fd, n, training=True, stats_out=stats),
               "pepnet": lambda s: O.pepnet_forward(s, X, fd, dom_idx, n, training=True, stats_out=stats),
               "epnet": lambda s: O.pepnet_forward(s, X, fd, dom_idx, n, training=True, stats_out=stats)}[name]
    elif name == "star":
        out, tt = model(xg, gg, targets=yg)
        fwd = lambda s: O.star_forward(s, X, fd, n, x_group=grp, targets=torch.from_numpy(y), training=True, stats_out=stats)[0]
        _, want_t = O.star_forward(sd, X, fd, n, x_group=grp, targets=torch.from_numpy(y), training=True, stats_out={})
        assert torch.equal(tt.cpu(), want_t.to(tt.dtype)), "reordered targets"
    elif name == "hinet":
        out, _ = model(xg, gg, targets=yg)
        fwd = lambda s: O.hinet_forward(s, X, fd, grp, dom_idx, training=True, stats_out=stats)
    else:
        centers = model.cluster_centers.detach().cpu().clone()
        out, tt = model(xg, None, targets=yg, is_training=True)
        fwd = lambda s: O.adl_forward(s, X, fd, centers, n, targets=torch.from_numpy(y), is_training=True, training=True,
                                      stats_out=stats)[0]
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    model.zero_grad()
    out.backward(gout.to(cuda))
    stats.clear()
    ref, grads = oracle_grads(fwd, sd, gout)
    assert_close(out, ref.reshape(out.shape), F32_RTOL, F32_ATOL, f"{name}-{n} predictions")
    # a tower with one row skips its BatchNorm (star.py:134-135, adl.py): its pre-BN bias has a real gradient, compared as such
    params = dict(model.named_parameters())
    names = list(sd)
    # (the rows of the grouped models are partitioned by tower; elsewhere every tower normalises the whole batch)
    def skipped(k, g):
        if name not in ("star", "adl") or g is None or not is_pre_bn_bias(k, set(names)):
            return False
        wk = {"shared_bn_bias": "shared_bn_weight"}.get(k, k[:-5] + ".weight")
        return float(g.abs().max()) > 1e-3 * max(float(grads[wk].abs().max()), 1e-3) + 1e-4   # above compare_param_grads' ~0
    for k in [k for k, g in grads.items() if skipped(k, g)]:
        assert_close(params[k].grad, grads.pop(k), MANY_RTOL, MANY_ATOL, f"grad {k} (BatchNorm skipped)")
    compare_param_grads(params, grads, MANY_RTOL, MANY_ATOL, all_names=names)
    new_sd = sd_cpu(model)
    for k, v in stats.items():
        assert_close(new_sd[k], v, F32_RTOL, F32_ATOL, f"stat {k}")


BF16_RTOL, BF16_ATOL = 5e-3, 2e-3       # the bf16 bounds of test_gpu_ple.py (against the oracle's exact bf16 restatement)


@pytest.mark.parametrize("name,n", [("ple", 25), ("ple", 50), ("hinet", 25), ("mmoe", 50)])
def test_model_at_many_towers_bf16_matches_oracle(cuda, name, n):
    """The default precision with the reference's dims (config.py): the bf16-shadow contractions, the grad-input split over
    several launches that add, and the wide pooling kernels' bf16 shadows, against the oracle's restatement of the bf16 path
    (operands of every contraction rounded to bf16, exact accumulation) under the bounds every bf16 path is held to."""
    from cdcmdr_amd.model.hinet import HiNet
    from cdcmdr_amd.model.mmoe import MMoE
    from cdcmdr_amd.model.ple import PLE
    # HiNet's domain-specific experts only see their domain's rows: 2048 rows give them ~80 each, as PLE's 512 give a tower
    B, dom_idx = (2048 if name == "hinet" else 512), 3
    fd = [1000] * 26
    fd[dom_idx] = n
    torch.manual_seed(n + 1)
    if name == "ple":
        model = PLE(fd, 16, n, 2, 2, ((256, 128), (64,)), (64, 32), dropout=0.0, config=CFG)
    elif name == "mmoe":
        model = MMoE(fd, 16, n, 4, (256, 128, 64), (64, 32), dropout=0.0, config=CFG)
    else:
        model = HiNet(fd, 16, n_tower=n, sei_dims=(64, 32), tower_dims=(256, 128, 64, 32), domain_idx=dom_idx, device="cuda",
                      dropout=0.0, config=CFG)
    model = model.to(cuda).set_precision("bf16").train()
    sd = sd_cpu(model)
    rng = np.random.default_rng(200 + n)
    X = make_ids(rng, B, fd)
    grp = _groups(rng, B, n)
    X[:, dom_idx] = grp
    xg, gg = torch.from_numpy(X).to(cuda), torch.from_numpy(grp).to(cuda)
    out = model(xg, gg, targets=None)[0] if name == "hinet" else model(xg)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    model.zero_grad()
    out.backward(gout.to(cuda))
    stats = {}
    fwd = {"ple": lambda s: O.ple_forward(s, X, fd, n, training=True, stats_out=stats),
           "mmoe": lambda s: O.mmoe_forward(s, X, fd, n, training=True, stats_out=stats),
           "hinet": lambda s: O.hinet_forward(s, X, fd, grp, dom_idx, training=True, stats_out=stats)}[name]
    O.MATMUL_BF16 = "exact"
    try:
        ref, grads = oracle_grads(fwd, sd, gout)
    finally:
        O.MATMUL_BF16 = False
    assert_close(out, ref.reshape(out.shape), BF16_RTOL, BF16_ATOL, f"{name}-{n} bf16 predictions")
    # the bounds the existing many-tower bf16 tests state (test_gpu_gaps.py STAR-30, test_gpu_cgc_mid.py PLE with 5-7 towers):
    # compare_param_grads' per-tensor bounds are stated for 3 towers; with 25-50 a single row's relu flip weighs more in the small
    # gradient of one tower's (or one domain's expert's) tensors, so the median and nine tensors in ten are the check and a
    # single tensor may reach 2.5e-1.  Pre-BN biases (a zero sum of bf16-rounded dZ) must be finite and small next to their weight.
    names = set(sd)
    params = dict(model.named_parameters())
    for k in [k for k in grads if grads[k] is not None and is_pre_bn_bias(k, names)]:
        grads.pop(k)
        got = params[k].grad
        wscale = float(params[k[:-5] + ".weight"].grad.abs().max())
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 2e-1 * max(wscale, 1e-3) + 1e-4, k
    compare_param_grads(params, grads, BF16_RTOL, BF16_ATOL, bf16=True, all_names=list(sd), max_rel=2.5e-1, p90_rel=5e-2)
    new_sd = sd_cpu(model)
    for k, v in stats.items():
        assert_close(new_sd[k], v, BF16_RTOL, BF16_ATOL, f"stat {k}")


# ------------------------------------------------------------------------------------------------------------------------
# the training step: graph = eager, dense table = lazy table (exact replay), bit for bit
# ------------------------------------------------------------------------------------------------------------------------
def _train(cuda, name, n, table_mode, use_graph, steps=3):
    from cdcmdr_amd.model.hinet import HiNet
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.model.star import STAR
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    B, dom_idx = 1024, 4
    fd = [50, 3000, 11, 700, n, 29]
    torch.manual_seed(3)
    if name == "ple":
        model, mode = PLE(fd, 16, n, 2, 2, ((256, 128), (64,)), (64, 32), dropout=0.2, config=CFG), "multi"
    elif name == "star":
        model, mode = STAR(fd, 16, n, (64, 32, 16), domain_idx=dom_idx, dropout=0.2, config=CFG), "star"
    else:
        model, mode = HiNet(fd, 16, n_tower=n, sei_dims=(64, 32), tower_dims=(256, 128, 64, 32), domain_idx=dom_idx, device="cuda",
                            dropout=0.2, config=CFG), "single_group"
    model = model.to(cuda)
    kw = {"fast_replay": False} if table_mode == "lazy" else {}
    opt = FusedAdam(model, table_mode=table_mode, **kw)
    ts = TrainStep(model, opt, B, mode=mode, use_graph=use_graph)
    rng = np.random.default_rng(21)
    losses = []
    batches = []
    for _ in range(steps + 1):
        X = make_ids(rng, B, fd)
        X[:, dom_idx] = _groups(rng, B, n)
        batches.append((torch.from_numpy(X).to(cuda), torch.from_numpy(rng.integers(0, 2, size=B).astype(np.int16)).to(cuda),
                        torch.from_numpy(X[:, dom_idx].astype(np.int64)).to(cuda)))
    for s in range(steps):
        X, y, g = batches[s]
        bce, _ = ts.step(X, y, g, next_X=batches[s + 1][0])
        losses.append(bce.detach().clone())
    if table_mode == "lazy":
        opt.flush_table()
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), sd_cpu(model)


@pytest.mark.parametrize("name,n", [("ple", 25), ("ple", 50), ("star", 50), ("hinet", 25)])
def test_train_step_graph_eager_dense_lazy_bit_identical(cuda, name, n):
    base_l, base_sd = _train(cuda, name, n, "dense", False)
    assert torch.isfinite(base_l).all()
    for table_mode, use_graph in [("dense", True), ("lazy", False)]:
        l, sd = _train(cuda, name, n, table_mode, use_graph)
        assert torch.equal(l, base_l), f"{name}-{n} {table_mode} graph={use_graph}: losses {l} vs {base_l}"
        for k, v in base_sd.items():
            assert torch.equal(sd[k], v), f"{name}-{n} {table_mode} graph={use_graph}: {k} differs"


def test_train_step_three_steps_match_oracle_ple25(cuda):
    """PLE-25 in fp32: three TrainStep steps equal the oracle's forward + torch.optim.Adam with the reference's settings."""
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    n, B = 25, 512
    fd = [11, 300, 5, 40, 3, 17]
    torch.manual_seed(4)
    model = PLE(fd, 8, n, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.0, config=CFG).to(cuda).set_precision("f32")
    sd0 = sd_cpu(model)
    opt = FusedAdam(model, table_mode="dense")
    ts = TrainStep(model, opt, B, mode="multi")
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd0.items() if v.dtype.is_floating_point and "running_" not in k}
    ref_opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-8)
    l2 = {k: 1e-5 for k in O.reg_names(list(sd0), "ple")}
    rng = np.random.default_rng(8)
    for _ in range(3):
        X = make_ids(rng, B, fd)
        g = _groups(rng, B, n)
        y = rng.integers(0, 2, size=B).astype(np.int16)
        bce, _ = ts.step(torch.from_numpy(X).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(g).to(cuda))
        s2 = dict(sd0)
        s2.update(leaves)
        p = O.ple_forward(s2, X, fd, n, training=True).gather(1, torch.from_numpy(g).reshape(-1, 1)).squeeze(1)
        want = O.bce_mean(p, torch.from_numpy(y))
        ref_opt.zero_grad()
        (want + O.reg_loss(s2, l2).sum()).backward()
        ref_opt.step()
        assert abs(float(bce.item()) - float(want.detach())) < 1e-4 * max(1.0, abs(float(want.detach())))
    got = sd_cpu(model)
    for k, leaf in leaves.items():
        if is_pre_bn_bias(k, set(sd0)):
            continue                        # a zero gradient up to rounding noise, which Adam scales to +-lr (as the golden tests)
        assert_close(got[k], leaf.detach(), 1e-3, 2e-5, k)


# ------------------------------------------------------------------------------------------------------------------------
# evaluation at 50 domains
# ------------------------------------------------------------------------------------------------------------------------
def test_evaluator_multi_at_50_domains(cuda):
    from cdcmdr_amd.evaluate import Evaluator
    from cdcmdr_amd.model.ple import PLE
    n, B, dom_idx = 50, 2000, 2
    fd = list(FD)
    fd[dom_idx] = n
    torch.manual_seed(6)
    model = PLE(fd, 4, n, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.0, config=CFG).to(cuda).set_precision("f32")
    rng = np.random.default_rng(6)
    batches = []
    for _ in range(3):
        X = make_ids(rng, B, fd)
        X[:, dom_idx] = rng.integers(0, n, size=B)
        y = rng.integers(0, 2, size=B).astype(np.int16)
        batches.append((torch.from_numpy(X).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(X[:, dom_idx].astype(np.int64)).to(cuda)))
    ev = Evaluator(model, mode="multi", domain_idx=dom_idx, n_domain=n)
    pred, label, domain = ev.predict(batches)
    model.eval()
    with torch.no_grad():
        direct = torch.cat([model(X).gather(1, g.reshape(-1, 1)).squeeze(1) for X, _, g in batches])
    assert torch.equal(pred.reshape(-1), direct.reshape(-1))
    res = ev.test(batches)
    p, t = pred.double().cpu().numpy(), label.cpu().numpy()
    assert abs(res["total_auc"] - O.auc(t, p)) < 1e-6
    assert abs(res["total_loss"] - O.logloss(t, p)) < 1e-5
    dom = domain.cpu().numpy()
    assert len(res["domain_auc"]) == n
    for d in (0, 17, 49):
        m = dom == d
        assert abs(res["domain_auc"][d] - O.auc(t[m], p[m])) < 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# plans within the older limits pick the same launches as before
# ------------------------------------------------------------------------------------------------------------------------
PLE3_FWD = ["cdc_weight_shadows", "cdc_embed_gather_fwd", "cdc_glinear_pair_fwd", "cdc_cgc_mid_fwd", "host"]
PLE3_BWD = ["host", "cdc_cgc_mid_bwd", "cdc_glinear_bwd_x", "cdc_glinear_bwd_x", "cdc_glinear_bwd_w"]
_SF = ["cdc_star_fuse_fwd", "cdc_star_fuse_fwd"]
_SB = ["cdc_star_fuse_bwd", "cdc_star_fuse_bwd"]
STAR30_FWD = (["cdc_embed_gather_fwd", "cdc_group_partition", "cdc_rows_permute", "cdc_rowdot_fwd"] + _SF + ["cdc_bn_fwd"] * 2 +
              3 * (_SF + ["cdc_glinear_fwd", "cdc_bn_fwd", "cdc_bn_fwd"]) + _SF + ["cdc_rowdot_fwd"])
STAR30_BWD = (["cdc_transpose_multi", "cdc_transpose_multi", "cdc_rowdot_bwd", "host"] +
              3 * (_SB + ["cdc_bn_bwd", "cdc_bn_bwd", "cdc_glinear_bwd_w", "cdc_glinear_bwd_x"]) + _SB + ["cdc_bn_bwd"] * 2 + _SB +
              ["cdc_rowdot_bwd", "cdc_rows_permute"])


def _names(steps):
    return [getattr(s, "what", "host") for s in steps]


def test_plans_within_the_old_limits_keep_their_launches(cuda):
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.model.star import STAR
    m = PLE([1000] * 26, 16, 3, 2, 2, ((256, 128), (64,)), (64, 32), 0.2, CFG).to(cuda).train()
    p = m.plan_holder(4096).plan
    assert _names(p.fwd_steps) == PLE3_FWD and _names(p.bwd_steps) == PLE3_BWD
    m = STAR([50, 3000, 11, 700, 30, 29], 16, 30, (64, 32, 16), domain_idx=4, dropout=0.0).to(cuda).train()
    p = m.plan_holder(1024, tag="grouped", grouped=True).plan
    assert _names(p.fwd_steps) == STAR30_FWD and _names(p.bwd_steps) == STAR30_BWD
