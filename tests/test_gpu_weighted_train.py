"""Training with loss weights on the fast path: TrainStep(..., loss_weights=LossWeights(...)) + step(..., weight=).

The weighted loss is torch's F.binary_cross_entropy(p, y, weight=w, reduction='mean') with the effective row weight
w = (row * domain_weight[X[:, domain_idx]]) * (pos_weight if y > 0 else 1), formed in fp32 in that order.  Checked here: parity with
the CPU oracle driven by torch autograd + torch's Adam in the multi, mean and star modes (set-up and tolerances of
tests/test_gpu_train.py); on a bf16 model whose towers take the fused launches, graph replay == eager, run-to-run determinism,
all-ones weights == the unweighted step, lazy == dense table; a weighted and an unweighted step sharing one cached plan; two
data-parallel ranks == one rank on the concatenated weighted batch; the argument errors."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from helpers import O, assert_close, is_pre_bn_bias, make_ids
from test_gpu_dist import B_LOCAL, FD, ROOT, STEPS, _build, _data, _free_port

pytestmark = pytest.mark.gpu
FD_SPARSE = [7, 400, 3, 50, 11, 29]
DOM_W3 = [0.5, 2.0, 1.25]
POS_W = 2.5


def w_eff(row, dom_ids, dom_w, y, pos_weight):
    """the contract's effective weight on the host: fp32, (row * dom) * pos"""
    row = np.asarray(row, dtype=np.float32).reshape(-1)
    dom = np.asarray(dom_w, dtype=np.float32)[np.asarray(dom_ids).reshape(-1)]
    pos = np.where(np.asarray(y).reshape(-1) > 0, np.float32(pos_weight), np.float32(1)).astype(np.float32)
    return ((row * dom).astype(np.float32) * pos).astype(np.float32)


def row_weights(rng, n):
    w = rng.uniform(0.0, 3.0, size=n).astype(np.float32)
    w[7::8] = 0.0
    return w


# ------------------------------------------------------------------------------------------------------------------------
# oracle parity: PLE, fp32, batches of 32, 32 and 16 rows through train_epoch, dense table
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["multi", "mean"])
def test_weighted_epoch_matches_the_oracle(cuda, mode):
    from cdcmdr_amd.data import make_loader, train_epoch
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import LossWeights, TrainStep
    fd = FD_SPARSE
    torch.manual_seed(21)
    model = PLE(fd, 4, 3, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.0).to(cuda).set_precision("f32")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(8)
    n = 80
    X = torch.from_numpy(make_ids(rng, n, fd))
    X[:, 2] = torch.from_numpy(rng.integers(0, 3, size=n).astype(np.int32))
    y = torch.from_numpy(rng.integers(0, 2, size=(n, 1)).astype(np.int16))
    rw = row_weights(rng, n)
    loader, _ = make_loader(X, y, 32, cuda, domain_idx=2, domain2group={0: 0, 1: 1, 2: 2}, shuffle=False, row_weight=torch.from_numpy(rw))
    assert loader.has_weight
    opt = FusedAdam(model, table_mode="dense")          # dense: the logged regularisation value is exact every step
    ts = TrainStep(model, opt, 32, mode=mode, loss_weights=LossWeights(row=True, domain_weight=DOM_W3, domain_idx=2, pos_weight=POS_W))
    logged = []
    done, skipped = train_epoch(ts, loader, log_interval=1, log=logged.append)
    assert (done, skipped) == (3, 0) and len(logged) == 3
    opt.flush_table()
    we = torch.from_numpy(w_eff(rw, X[:, 2].numpy(), DOM_W3, y.numpy(), POS_W))
    # the oracle: same batches, torch.optim.Adam on the CPU, torch's own weighted BCE
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
    s2 = dict(sd)
    s2.update(leaves)
    l2 = {k: 1e-5 for k in O.reg_names(list(sd), "ple")}
    ref_opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-8)
    names = set(sd)
    want_losses = []
    for lo in (0, 32, 64):
        xb, yb = X[lo:lo + 32].numpy(), y[lo:lo + 32, 0].float()
        gb = X[lo:lo + 32, 2].to(torch.int64).reshape(-1, 1)
        stats = {}
        out = O.ple_forward(s2, xb, fd, 3, training=True, stats_out=stats)
        p = out.mean(dim=1) if mode == "mean" else out.gather(1, gb).squeeze(1)
        loss = F.binary_cross_entropy(p, yb, weight=we[lo:lo + 32]) + O.reg_loss(s2, l2)
        ref_opt.zero_grad()
        loss.sum().backward()
        ref_opt.step()
        want_losses.append(float(loss.sum().detach()))
        s2.update(stats)
    got = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    print("logged", logged, "want", want_losses)
    for a, b in zip(logged, want_losses):
        assert abs(a - b) < 2e-5 * max(1.0, abs(b)), (logged, want_losses)
    for k in names:
        if is_pre_bn_bias(k, names) or "num_batches" in k:
            continue
        atol = 1.5e-3 if k.endswith("running_mean") else 2e-5
        assert_close(got[k], s2[k].detach(), 5e-4, atol, f"weighted epoch ({mode}): {k}")


def test_weighted_star_fast_path_matches_the_oracle(cuda):
    """mode="star": the weights follow the labels through the partition's row order"""
    from cdcmdr_amd.model.star import STAR
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import LossWeights, TrainStep
    fd = [7, 400, 3, 50, 5, 29]
    dom_w = [0.5, 2.0, 1.25, 3.0, 0.75]
    torch.manual_seed(9)
    model = STAR(fd, 4, 5, (32, 16, 8), domain_idx=4, dropout=0.0).to(cuda).set_precision("f32")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    opt = FusedAdam(model, table_mode="dense")
    ts = TrainStep(model, opt, 96, mode="star", loss_weights=LossWeights(row=True, domain_weight=dom_w, domain_idx=4, pos_weight=POS_W))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
    s2 = dict(sd)
    s2.update(leaves)
    l2 = {k: 1e-5 for k in O.reg_names(list(sd), "star")}
    ref_opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-8)
    rng = np.random.default_rng(6)
    names = set(sd)
    for step in range(2):
        X = make_ids(rng, 96, fd)
        if step == 1:
            X[X[:, 4] == 3, 4] = 2                                  # domain 3 absent
        y = rng.integers(0, 2, size=96).astype(np.int16)
        rw = row_weights(rng, 96)
        g = X[:, 4].astype(np.int64)
        bce, _ = ts.step(torch.from_numpy(X).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(g).to(cuda),
                         weight=torch.from_numpy(rw).to(cuda))
        stats = {}
        p, t = O.star_forward(s2, X, fd, 5, x_group=g, targets=torch.from_numpy(y).float(), training=True, stats_out=stats)
        order = np.argsort(g, kind="stable")                        # ascending group, original order inside a group
        assert np.array_equal(t.numpy(), y[order].astype(np.float32))
        we = torch.from_numpy(w_eff(rw, g, dom_w, y, POS_W)[order])
        bce_ref = F.binary_cross_entropy(p.squeeze(1), t, weight=we)
        loss = bce_ref + O.reg_loss(s2, l2)
        ref_opt.zero_grad()
        loss.sum().backward()
        if step == 0:
            used = {k for k, leaf in leaves.items() if leaf.grad is not None}
        for k, leaf in leaves.items():
            if leaf.grad is None and k in used:
                leaf.grad = torch.zeros_like(leaf)
        ref_opt.step()
        s2.update(stats)
        assert abs(float(bce.item()) - float(bce_ref.detach())) < 2e-5
    got = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for k in names:
        if "num_batches" in k or is_pre_bn_bias(k, names):
            continue
        if k == "shared_bn_bias" or (k.startswith("domain_norm.") and k.endswith(".bias")):
            continue
        atol = 5e-4 if k.endswith("running_mean") else 2e-5
        assert_close(got[k], s2[k].detach(), 5e-4, atol, f"weighted star step: {k}")


# ------------------------------------------------------------------------------------------------------------------------
# a bf16 model whose towers take the fused launches
# ------------------------------------------------------------------------------------------------------------------------
DOM_W_FD = [0.5, 2.0, 1.25]                     # FD's field 4 has three ids


def _ple64(cuda):
    from cdcmdr_amd.model.ple import PLE
    torch.manual_seed(5)
    return PLE(FD, 8, 3, 1, 1, ((32,), (64,)), (64, 32), dropout=0.0).to(cuda).set_precision("bf16")


def _batches(cuda, n_steps, B, ones=False):
    r = np.random.default_rng(31)
    out = []
    for _ in range(n_steps):
        X = make_ids(r, B, FD)
        y = r.integers(0, 2, size=B).astype(np.int16)
        w = row_weights(r, B)                                       # a different weight vector every step
        if ones:                                                    # (drawn all the same: the batches do not depend on `ones`)
            w = np.ones(B, dtype=np.float32)
        out.append(tuple(torch.from_numpy(a).to(cuda) for a in (X, y, X[:, 4].astype(np.int64), w)))
    return out


def _state(model, opt, losses):
    """parameters and running statistics, the table and every Adam moment, on the host"""
    opt.flush_table()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sd["table_m"], sd["table_v"] = opt.table_m.cpu().clone(), opt.table_v.cpu().clone()
    for name, st in opt.state_dict()["state"].items():
        sd[name + "/exp_avg"], sd[name + "/exp_avg_sq"] = st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()
    return sd, list(losses)


def _run_ple64(cuda, weights, n_steps=4, use_graph=False, table_mode="lazy", ones=False, B=64):
    """weights: a LossWeights or None (then the batches' weight is not passed)"""
    from cdcmdr_amd import plan as P
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    model = _ple64(cuda)
    opt = FusedAdam(model, table_mode=table_mode, fast_replay=False, flush_every=0)
    ts = TrainStep(model, opt, B, use_graph=use_graph, loss_weights=weights)
    losses = []
    for X, y, g, w in _batches(cuda, n_steps, B, ones=ones):
        bce, _ = ts.step(X, y, g, weight=w) if (weights is not None and weights.row) else ts.step(X, y, g)
        losses.append(float(bce.item()))
    assert any(isinstance(op, P.TowerChain) for op in ts.plan.ops), "the fused tower launches were not chosen"
    assert ts._fuse_bce and ts._tower_both is not None, "the loss (weighted or not) is formed inside the towers' one launch"
    if use_graph:
        assert ts.graph is not None
    ts.check_ids()
    return _state(model, opt, losses)


def _same(a, b, what):
    assert a[1] == b[1], f"{what}: losses {a[1]} vs {b[1]}"
    assert all(np.isfinite(a[1]))
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), f"{what}: {k} differs"


def _lw(**kw):
    from cdcmdr_amd.trainer import LossWeights
    return LossWeights(**kw)


def test_fused_tower_model_graph_equals_eager_and_is_deterministic(cuda):
    lw = dict(row=True, domain_weight=DOM_W_FD, domain_idx=4, pos_weight=POS_W)
    eager = _run_ple64(cuda, _lw(**lw))
    _same(eager, _run_ple64(cuda, _lw(**lw)), "run to run")
    _same(eager, _run_ple64(cuda, _lw(**lw), use_graph=True), "graph replay vs eager")
    # the weights matter: the unweighted run is another trajectory
    assert eager[1] != _run_ple64(cuda, None)[1]


def test_all_ones_weights_equal_the_unweighted_step(cuda):
    plain = _run_ple64(cuda, None, n_steps=3)
    ones = _run_ple64(cuda, _lw(row=True), n_steps=3, ones=True)
    _same(ones, plain, "all-ones weight= vs a TrainStep built without weights")


def test_lazy_and_dense_table_are_bit_identical_with_weights(cuda):
    lw = dict(row=True, domain_weight=DOM_W_FD, domain_idx=4, pos_weight=POS_W)
    lazy, dense = _run_ple64(cuda, _lw(**lw), n_steps=6), _run_ple64(cuda, _lw(**lw), n_steps=6, table_mode="dense")
    for k in ("embedding.embedding_dict.weight", "table_m", "table_v"):
        assert torch.equal(lazy[0][k], dense[0][k]), f"table {k}: lazy replay differs from the dense pass"


def test_weighted_and_unweighted_steps_share_one_plan(cuda):
    """A weighted and an unweighted TrainStep on one model and optimiser share the cached plan and with it the argument blocks.
    Stepped alternately, each must behave as it does alone: the run equals, bit for bit, ONE weighted step object that is given the
    host-formed effective weights on the even steps and all-ones weights on the odd ones (all-ones == unweighted is the test above).
    A weight pointer left behind for the unweighted step, or missing for the weighted one, changes the trajectory."""
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    B, n = 64, 6
    batches = _batches(cuda, n, B)

    def run(shared):
        model = _ple64(cuda)
        opt = FusedAdam(model, table_mode="lazy", fast_replay=False, flush_every=0)
        if shared:
            tw = TrainStep(model, opt, B, loss_weights=_lw(row=True, domain_weight=DOM_W_FD, domain_idx=4, pos_weight=POS_W))
            tu = TrainStep(model, opt, B)
            assert tw.plan is tu.plan, "the two steps were expected to share the cached plan"
        else:
            one = TrainStep(model, opt, B, loss_weights=_lw(row=True))
        losses = []
        for i, (X, y, g, w) in enumerate(batches):
            if shared:
                bce, _ = tw.step(X, y, g, weight=w) if i % 2 == 0 else tu.step(X, y, g)
            else:
                we = w_eff(w.cpu().numpy(), X[:, 4].cpu().numpy(), DOM_W_FD, y.cpu().numpy(), POS_W) if i % 2 == 0 else np.ones(B, dtype=np.float32)
                bce, _ = one.step(X, y, g, weight=torch.from_numpy(we).to(cuda))
            losses.append(float(bce.item()))
        return _state(model, opt, losses)

    _same(run(True), run(False), "alternating on a shared plan vs one step object given the same effective weights")


# ------------------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on one GPU == one rank on the concatenated weighted batch
# ------------------------------------------------------------------------------------------------------------------------
def _dp_weights(world):
    """Per-row weights, uniform [0, 2) with every eighth exactly 0: their mean is about 1, so the gradients have the scale of the
    unweighted runs whose tolerances this test takes over.  That matters for one thing only: the bias of a Linear in front of a
    BatchNorm has a mathematically zero gradient, Adam turns its rounding noise into moves of up to +-lr per step (less the smaller
    the noise is against eps), and the running means carry those moves — weights that scale every gradient up scale that noise up."""
    w = np.random.default_rng(77).uniform(0.0, 2.0, size=B_LOCAL * world * STEPS).astype(np.float32)
    w[7::8] = 0.0
    return w


def _dp_loss_weights():
    from cdcmdr_amd.trainer import LossWeights
    return LossWeights(row=True)


def _dp_worker(rank, world, port, out_dir, kind):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    sys.path.insert(0, ROOT)
    from cdcmdr_amd import plan as P
    from cdcmdr_amd.dist import DataParallel
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    dev = torch.device("cuda:0")
    dp = DataParallel(backend="gloo")
    torch.manual_seed(5)
    model, mode = _build(kind, dev)
    opt = FusedAdam(model, table_mode="lazy", flush_every=2)
    ts = TrainStep(model, opt, B_LOCAL, mode=mode, dist=dp, table_dist="sharded", loss_weights=_dp_loss_weights())
    X, y, g = _data(world)
    w = _dp_weights(world)
    gb = B_LOCAL * world
    losses = []
    for s in range(STEPS):
        lo = s * gb + rank * B_LOCAL
        sl = slice(lo, lo + B_LOCAL)                                # each rank stages the weights of its own rows
        bce, _ = ts.step(*(torch.from_numpy(a[sl]).to(dev) for a in (X, y, g)), weight=torch.from_numpy(w[sl]).to(dev))
        losses.append(float(bce.item()))
    if kind == "ple64":
        assert any(isinstance(op, P.TowerChain) for op in ts.plan.ops), "the fused tower launches were not chosen"
    ts.check_ids()
    ts.gather_table()
    torch.save({"sd": {k: v.cpu() for k, v in model.state_dict().items()}, "m": opt.table_m.cpu(), "losses": losses},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dp.barrier()
    dp.close()


def _dp_single(kind, world):
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    model, mode = _build(kind, dev)
    opt = FusedAdam(model, table_mode="lazy", flush_every=2)
    gb = B_LOCAL * world
    ts = TrainStep(model, opt, gb, mode=mode, loss_weights=_dp_loss_weights())
    X, y, g = _data(world)
    w = _dp_weights(world)
    losses = []
    for s in range(STEPS):
        sl = slice(s * gb, (s + 1) * gb)
        bce, _ = ts.step(*(torch.from_numpy(a[sl]).to(dev) for a in (X, y, g)), weight=torch.from_numpy(w[sl]).to(dev))
        losses.append(float(bce.item()))
    opt.flush_table()
    return {k: v.cpu() for k, v in model.state_dict().items()}, losses


@pytest.mark.parametrize("kind", ["mmoe", "ple64"])
def test_two_ranks_equal_one_rank_on_the_concatenated_weighted_batch(cuda, tmp_path, kind):
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), kind), nprocs=world, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world))
    assert r0["losses"] == r1["losses"] and all(np.isfinite(r0["losses"]))
    for k in r0["sd"]:
        assert torch.equal(r0["sd"][k], r1["sd"][k]), f"replicas diverged in {k}"
    assert torch.equal(r0["m"], r1["m"])
    ref_sd, ref_losses = _dp_single(kind, world)
    print("losses", r0["losses"], ref_losses)
    names = set(ref_sd)
    for a, b in zip(r0["losses"], ref_losses):
        assert abs(a - b) < (1e-5 if kind == "ple64" else 2e-5), (r0["losses"], ref_losses)
    for k, v in ref_sd.items():
        if is_pre_bn_bias(k, names) or "num_batches" in k:
            continue
        if kind == "ple64":            # test_ranks_with_the_fused_towers_split_around_the_batchnorm_exchanges
            d = float((r0["sd"][k].double() - v.double()).abs().max())
            assert d < 2e-4, f"2-rank split towers vs 1-rank monolithic towers: {k}: {d:.3e}"
        else:                          # test_two_ranks_stay_identical
            atol = 5e-4 if k.endswith("running_mean") else 2e-5
            assert_close(r0["sd"][k], v, 5e-4, atol, f"2-rank vs 1-rank: {k}")


# ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(cuda):
    from cdcmdr_amd.model.mmoe import MMoE
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import LossWeights, TrainStep
    fd = [20, 500, 7, 90, 4]
    model = MMoE(fd, 8, 3, 4, (32, 16), (8,), dropout=0.0).to(cuda).set_precision("f32")
    opt = FusedAdam(model, table_mode="dense")
    r = np.random.default_rng(1)
    X = torch.from_numpy(make_ids(r, 16, fd)).to(cuda)
    y = torch.from_numpy(r.integers(0, 2, size=16).astype(np.int16)).to(cuda)
    g = torch.from_numpy(r.integers(0, 3, size=16).astype(np.int64)).to(cuda)
    w = torch.ones(16, device=cuda)
    with pytest.raises(ValueError, match="needs weight="):
        TrainStep(model, opt, 16, loss_weights=LossWeights(row=True)).step(X, y, g)
    with pytest.raises(ValueError, match="without loss_weights"):
        TrainStep(model, opt, 16).step(X, y, g, weight=w)
    with pytest.raises(ValueError, match="row=False"):
        TrainStep(model, opt, 16, loss_weights=LossWeights(pos_weight=2.0)).step(X, y, g, weight=w)
    with pytest.raises(ValueError, match="holds 3 weights"):
        TrainStep(model, opt, 16, loss_weights=LossWeights(domain_weight=[1.0, 2.0, 3.0], domain_idx=4))
    with pytest.raises(ValueError, match="fp32"):
        TrainStep(model, opt, 16, loss_weights=LossWeights(row=True)).step(X, y, g, weight=torch.ones(15, device=cuda))
