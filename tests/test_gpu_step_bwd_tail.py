"""TrainStep(bwd_tail_one_launch=): the embeddings' grad-input launch and the batched grad-weight launch that end the backward
issued as ONE launch (cdc_glinear_bwd_xw) — the same training, byte for byte, as with the two launches.

The model is the PLE whose launch lists tests/test_gpu_many_domains.py pins (vocabulary 1000), at B = 512: the batched
grad-weight launches then run with split_k = 2, so the deferred slabs (summed by the closing Adam launch) are exercised.  Three
steps each way from one seed, eagerly and as a replayed graph; the plan's own step list is the pinned one either way (the fused
call is what the trainer issues in place of the last two entries, not an entry).  A plan whose tail has another form (the same
PLE in fp32: no shadows, no pair launch) keeps its two launches whatever the switch says, and trains."""
import types

import numpy as np
import pytest
import torch

from helpers import make_ids, sd_cpu

pytestmark = pytest.mark.gpu

CFG = types.SimpleNamespace(use_atten=False, use_dcn=False)
FD = [1000] * 26
B = 512
PLE3_BWD = ["host", "cdc_cgc_mid_bwd", "cdc_glinear_bwd_x", "cdc_glinear_bwd_x", "cdc_glinear_bwd_w"]
_RUNS = {}


def _names(steps):
    return [getattr(s, "what", "host") for s in steps]


def _train(cuda, one_launch, use_graph=False, precision="bf16", steps=3):
    """(fused?, bwd launch names, issued launch names of one eager step, losses, outputs, state_dict) — computed once per setting"""
    key = (one_launch, use_graph, precision)
    if key in _RUNS:
        return _RUNS[key]
    from cdcmdr_amd import _lib as L
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.trainer import TrainStep
    torch.manual_seed(3)
    model = PLE(FD, 16, 3, 2, 2, ((256, 128), (64,)), (64, 32), 0.2, CFG).to(cuda).train()
    model.set_precision(precision)
    opt = FusedAdam(model, table_mode="lazy")
    ts = TrainStep(model, opt, B, mode="multi", use_graph=use_graph, bwd_tail_one_launch=one_launch)
    rng = np.random.default_rng(21)
    batches = []
    for _ in range(steps + 1):
        X = make_ids(rng, B, FD)
        X[:, 10] %= 3
        batches.append((torch.from_numpy(X).to(cuda), torch.from_numpy(rng.integers(0, 2, size=B).astype(np.int16)).to(cuda),
                        torch.from_numpy(X[:, 10].astype(np.int64)).to(cuda)))
    losses, outs, issued = [], [], []
    for s in range(steps):
        X, y, g = batches[s]
        if s == 0 and not use_graph:
            rec = []
            L.PROFILE = rec                                           # (names of the launches this step issues)
        try:
            bce, _ = ts.step(X, y, g, next_X=batches[s + 1][0])
        finally:
            if s == 0 and not use_graph:
                L.PROFILE = None
                issued = [r[0] for r in rec]
        losses.append(bce.detach().clone())
        outs.append(ts.out.tensor().detach().clone())
    ts.gather_table()
    torch.cuda.synchronize()
    _RUNS[key] = (ts.bwd_tail_fused, _names(ts.plan.bwd_steps), issued, torch.stack(losses).cpu(), torch.stack(outs).cpu(), sd_cpu(model))
    return _RUNS[key]


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)), f"{what}: bytes differ"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_fused_tail_trains_byte_for_byte_like_two_launches(cuda, use_graph):
    fused, names1, issued1, loss1, out1, sd1 = _train(cuda, True, use_graph)
    plain, names0, issued0, loss0, out0, sd0 = _train(cuda, False, use_graph)
    assert fused is True and plain is False
    assert names1 == PLE3_BWD and names0 == PLE3_BWD
    if not use_graph:                                                 # what went out: one launch in place of two
        assert "cdc_glinear_bwd_xw" in issued1 and "cdc_glinear_bwd_w" not in issued1
        assert issued1.count("cdc_glinear_bwd_x") == issued0.count("cdc_glinear_bwd_x") - 1
        assert "cdc_glinear_bwd_xw" not in issued0 and issued0.count("cdc_glinear_bwd_w") == 1
        assert len(issued1) == len(issued0) - 1
    assert torch.isfinite(loss1).all() and float(loss1[0]) != float(loss1[-1])
    _same_bytes(loss1, loss0, "losses")
    _same_bytes(out1, out0, "outputs")
    assert sd1.keys() == sd0.keys()
    for k in sd1:
        _same_bytes(sd1[k], sd0[k], f"state_dict[{k}]")


def test_fused_graph_equals_eager(cuda):
    _, _, _, loss_e, out_e, sd_e = _train(cuda, True, False)
    _, _, _, loss_g, out_g, sd_g = _train(cuda, True, True)
    _same_bytes(loss_e, loss_g, "losses")
    _same_bytes(out_e, out_g, "outputs")
    for k in sd_e:
        _same_bytes(sd_e[k], sd_g[k], f"state_dict[{k}]")


def test_a_tail_of_another_form_keeps_its_two_launches(cuda):
    fused, names, issued, loss1, out1, sd1 = _train(cuda, True, precision="f32")
    assert fused is False
    assert "cdc_glinear_bwd_xw" not in issued and any(n.startswith("cdc_glinear_bwd_w") for n in issued)
    assert torch.isfinite(loss1).all() and float(loss1[0]) != float(loss1[-1])
    plain, names0, issued0, loss0, out0, sd0 = _train(cuda, False, precision="f32")
    assert plain is False and names == names0 and issued == issued0
    _same_bytes(loss1, loss0, "losses")
    for k in sd1:
        _same_bytes(sd1[k], sd0[k], f"state_dict[{k}]")
