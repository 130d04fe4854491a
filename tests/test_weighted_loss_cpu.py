"""Loss weights on the CPU: (a) the weighted float64 reference of the fused towers (tests/weighted_ref.py, a wrapper around
tower_ref.logit_gradients) chained with nothing rounded is torch autograd of F.binary_cross_entropy(weight=), within the bound
tests/test_tower_ref_cpu.py holds the unweighted chain to; (b) the weighted head reference with all-ones weights is
tests/test_gpu_head.py's unweighted one; (c) make_loader(row_weight=) keeps weight and row together through shuffling, rank shards and
the ragged tail; (d) LossWeights refuses what it cannot mean; (e) the new entry points refuse bad arguments without a launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_head as H
import test_tower_ref_cpu as TC
import tower_ref as R
import weighted_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TORCH_CASES = [c for c in TC.TORCH_CASES if R.bce(c)]


# ------------------------------------------------------------------------------------------------------------------------
# (a) the wrapped tower reference against torch autograd, float64
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TORCH_CASES, ids=[c["name"] for c in TORCH_CASES])
def test_the_weighted_chain_is_torch_autograd_of_the_weighted_loss(c, monkeypatch):
    D = R.make_data(c)
    w = W.weights(c["name"], c["M"])
    monkeypatch.setattr(R, "logit_gradients", W.tower_logit_gradients(w))      # ref_backward looks the name up at call time
    F = R.ref_forward(c, D, None)
    Bk = R.ref_backward(c, D, F["chained"], chain=True)
    # torch's side: the unweighted chain's tower with torch's own weight= in its loss
    bce = torch.nn.functional.binary_cross_entropy
    w64 = torch.from_numpy(w.astype(np.float64))
    monkeypatch.setattr(torch.nn.functional, "binary_cross_entropy", lambda p, y, reduction="mean": bce(p, y, weight=w64, reduction=reduction))
    T = TC._torch_tower(c, D)
    plain = R.ref_backward.__globals__["logit_gradients"]
    assert plain is not W._tower_logit_gradients                                # the wrapper is what ran
    seen = 0
    for k, want in T.items():
        have = F.get(k, Bk.get(k))
        assert have is not None, k
        a, b = np.asarray(have[0], dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
        err = float(np.max(np.abs(a - b))) if a.size else 0.0
        assert err <= 2e-12 * max(1.0, float(np.max(np.abs(b)))), f"{c['name']} {k}: {err:.3e}"
        seen += 1
    assert seen >= 10 * c["n_tower"]
    # and the weights matter: the unweighted chain is another result
    monkeypatch.setattr(R, "logit_gradients", W._tower_logit_gradients)
    U = R.ref_backward(c, D, F["chained"], chain=True)
    assert abs(float(U["loss"][0][0]) - float(Bk["loss"][0][0])) > 1e-3


def test_all_ones_weights_give_the_unweighted_tower_reference_and_a_wider_bound():
    c = R.by_name("rows129_bce")
    D = R.make_data(c)
    out = R.ref_forward(c, D, None)["chained"]["out"]
    d0, cd0, loss0 = W._tower_logit_gradients(c, D, out)
    d1, cd1, loss1 = W.tower_logit_gradients(np.ones(c["M"], dtype=np.float32))(c, D, out)
    assert np.array_equal(d0, d1) and cd1 == cd0 + 1
    assert loss1[0][0] == pytest.approx(loss0[0][0], rel=1e-15) and loss1[1][0] >= loss0[1][0]


# ------------------------------------------------------------------------------------------------------------------------
# (b) the weighted head reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gkind", ["none", "outside"])
def test_the_weighted_head_reference_with_all_ones_is_the_unweighted_one(gkind):
    s = dict(H._spec("d"), acc_dx=(0, 0), acc_wide=0, acc_add=(0,))            # plain stores: what weighted_ref.head_backward restates
    D = H.make_data(s, ("i16", gkind))
    out32 = H.ref_forward(s, D)["out"][0].astype(np.float32)
    want = H.ref_backward(s, D, out32, ("i16", gkind))
    M = s["M"]
    got = W.head_backward(s["K"], s["wide"], s["n_add"], D, out32, np.ones(M, dtype=np.float32), 1.0 / M)
    assert set(got) == {k for k, v in want.items() if isinstance(v, tuple)}
    for k, (v, b) in got.items():
        np.testing.assert_allclose(v, want[k][0], rtol=1e-14, atol=0)
        assert (b >= want[k][1] * (1 - 1e-12)).all(), k                          # one rounding more, never a tighter bound
    w = W.weights("head", M)
    scaled = W.head_backward(s["K"], s["wide"], s["n_add"], D, out32, w, 1.0 / M)
    np.testing.assert_allclose(scaled["dx0"][0], got["dx0"][0] * w[:, None].astype(np.float64), rtol=1e-14)
    assert not scaled["dx1"][0][w == 0].any()


# ------------------------------------------------------------------------------------------------------------------------
# (c) make_loader(row_weight=)
# ------------------------------------------------------------------------------------------------------------------------
def _rows(n=203, F=4):
    """every row carries its own index in field 0, and its weight is that index + 0.5"""
    X = torch.zeros(n, F, dtype=torch.int32)
    X[:, 0] = torch.arange(n, dtype=torch.int32)
    X[:, 2] = torch.arange(n, dtype=torch.int32) % 3
    y = (torch.arange(n) % 2).to(torch.int16).reshape(-1, 1)
    return X, y, torch.arange(n, dtype=torch.float32) + 0.5


def _check_batches(batches, with_group):
    seen = []
    for b in batches:
        assert len(b) == (4 if with_group else 3)
        X, w = b[0], b[-1]
        assert w.dtype == torch.float32 and w.shape == (X.shape[0], 1)
        assert torch.equal(w.reshape(-1), X[:, 0].float() + 0.5), "a weight left its row"
        assert torch.equal(b[1].reshape(-1), (X[:, 0] % 2).to(torch.int16))
        seen += X[:, 0].tolist()
    return seen


@pytest.mark.parametrize("with_group", [False, True])
def test_make_loader_keeps_weight_and_row_together(with_group):
    from cdcmdr_amd.data import make_loader
    X, y, w = _rows()
    kw = dict(domain_idx=2, domain2group={0: 0, 1: 1, 2: 2}) if with_group else {}
    torch.manual_seed(3)
    loader, _ = make_loader(X, y, 32, "cpu", shuffle=True, row_weight=w, **kw)
    assert loader.has_weight
    batches = list(loader)
    seen = _check_batches(batches, with_group)
    assert sorted(seen) == list(range(203)) and seen != list(range(203))        # shuffled, every row once
    assert batches[-1][0].shape[0] == 203 % 32                                   # the ragged tail carries its weights
    plain, _ = make_loader(X, y, 32, "cpu", shuffle=False, **kw)
    assert not plain.has_weight and len(next(iter(plain))) == (3 if with_group else 2)
    # the domain filter drops the weights of the rows it drops
    loader, _ = make_loader(X, y, 32, "cpu", domain_idx=2, domain_filter=[1], shuffle=False, row_weight=w)
    seen = _check_batches(list(loader), False)
    assert seen == [i for i in range(203) if i % 3 == 1]
    with pytest.raises(ValueError, match="row_weight"):
        make_loader(X, y, 32, "cpu", row_weight=w[:-1])


def test_rank_shards_and_the_ragged_tail_carry_their_weights():
    from cdcmdr_amd.data import make_loader
    X, y, w = _rows(n=2 * 3 * 16 + 11)
    world, seen = 3, []
    tails = []
    for rank in range(world):
        torch.manual_seed(5)
        loader, _ = make_loader(X, y, 16, "cpu", shuffle=True, rank=rank, world=world, row_weight=w)
        batches = list(loader)
        assert len(batches) == 3 and loader.last_global_rows == 11
        seen += _check_batches(batches, False)
        tails.append(batches[-1][0].shape[0])
    assert sorted(seen) == list(range(107)) and sorted(tails) == [3, 4, 4]


def test_train_epoch_hands_the_last_tensor_over_as_weight():
    """the look-ahead still takes batch[0] as the ids; the weight goes to step(weight=), never into the positional arguments"""
    from cdcmdr_amd.data import make_loader, train_epoch
    X, y, w = _rows(n=80)
    loader, _ = make_loader(X, y, 32, "cpu", domain_idx=2, domain2group={0: 0, 1: 1, 2: 2}, shuffle=False, row_weight=w)
    calls = []

    class Step:
        B, world, device = 32, 1, torch.device("cpu")

        def __init__(self, B=32):
            self.B = B

        def refresh_table_reg(self):
            pass

        def check_ids(self):
            pass

        def sibling(self, rows):
            return self.__dict__.setdefault("_siblings", {}).setdefault(rows, Step(rows))

        def step(self, X, y, group=None, next_X=None, *, weight=None):
            calls.append((X, y, group, next_X, weight))
            return torch.zeros(1), torch.zeros((), dtype=torch.float64)

    assert train_epoch(Step(), loader, log_interval=100) == (3, 0)
    assert [c[0].shape[0] for c in calls] == [32, 32, 16]
    for X_, y_, g_, nx, w_ in calls:
        assert g_ is not None and g_.dtype == torch.int64 and torch.equal(w_.reshape(-1), X_[:, 0].float() + 0.5)
    assert calls[0][3] is not None and torch.equal(calls[0][3], calls[1][0])    # the next batch's IDS were announced
    assert calls[1][3] is None and calls[2][3] is None                           # (the ragged batch is not announced)


# ------------------------------------------------------------------------------------------------------------------------
# (d) LossWeights
# ------------------------------------------------------------------------------------------------------------------------
def test_loss_weights_validation():
    from cdcmdr_amd.trainer import LossWeights
    assert not LossWeights().active and LossWeights(row=True).active and LossWeights(pos_weight=2.0).active
    lw = LossWeights(domain_weight=[1.0, 2.0, 0.5], domain_idx=2)
    assert lw.active and lw.domain_weight.dtype == torch.float32
    lw.check([10, 20, 3, 5])
    with pytest.raises(ValueError, match="holds 3 weights"):
        lw.check([10, 20, 4, 5])
    with pytest.raises(ValueError, match="not one of the model's"):
        lw.check([10, 20])
    with pytest.raises(ValueError, match="belong together"):
        LossWeights(domain_weight=[1.0])
    with pytest.raises(ValueError, match="belong together"):
        LossWeights(domain_idx=1)
    with pytest.raises(ValueError, match="finite"):
        LossWeights(pos_weight=float("inf"))
    with pytest.raises(ValueError, match="finite"):
        LossWeights(pos_weight=float("nan"))
    with pytest.raises(ValueError, match="finite"):
        LossWeights(domain_weight=[1.0, float("nan")], domain_idx=0)
    with pytest.raises(ValueError, match="field index"):
        LossWeights(domain_weight=[1.0], domain_idx=-1)


# ------------------------------------------------------------------------------------------------------------------------
# (e) the new entry points refuse bad arguments before any launch
# ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(16)                                    # a non-null address that is never dereferenced on the host
    # weighted BCE: NULL weight, NULL p / loss / labels, bad sizes
    for args in [(one, 1, None, one, None, None, one, None, 0, 4, 1, 1.0),            # weight NULL
                 (None, 1, None, one, None, one, one, None, 0, 4, 1, 1.0),            # p NULL
                 (one, 1, None, None, None, one, one, None, 0, 4, 1, 1.0),            # no labels
                 (one, 1, None, one, None, one, None, None, 0, 4, 1, 1.0),            # loss NULL
                 (one, 1, None, one, None, one, one, None, 0, 0, 1, 1.0),             # B = 0
                 (one, 2, None, one, None, one, one, None, 0, 4, 3, 1.0),             # ldp < n_col
                 (one, 3, None, one, None, one, one, one, 2, 4, 3, 1.0)]:             # lddp < n_col
        assert lib.cdc_bce_weighted_fwd_bwd(*args, None) < 0 and b"bce_weighted_fwd_bwd" in lib.cdc_last_error()
    for args in [(one, 1, one, None, None, one, None, 0, 4, 1, 1.0),                  # weight NULL
                 (one, 1, None, None, one, one, None, 0, 4, 1, 1.0),                  # no labels
                 (one, 1, one, None, one, one, None, 0, 4, 0, 1.0),                   # n_col = 0
                 (one, 2, one, None, one, one, one, 2, 4, 3, 1.0)]:                   # ldp, lddp < n_col
        assert lib.cdc_bce_mean_weighted_fwd_bwd(*args, None) < 0 and b"bce_mean_weighted_fwd_bwd" in lib.cdc_last_error()
    # weight staging: w_out NULL, B = 0, pos_weight != 1 without labels, not finite, a domain table without ids / column / length
    for args in [(None, None, 0, 0, None, 0, None, 1.0, None, 4),
                 (None, None, 0, 0, None, 0, None, 1.0, one, 0),
                 (None, None, 0, 0, None, 0, None, 2.0, one, 4),
                 (None, None, 0, 0, None, 0, one, float("inf"), one, 4),
                 (None, None, 5, 2, one, 3, None, 1.0, one, 4),
                 (None, one, 5, 5, one, 3, None, 1.0, one, 4),
                 (None, one, 5, -1, one, 3, None, 1.0, one, 4),
                 (None, one, 5, 2, one, 0, None, 1.0, one, 4)]:
        assert lib.cdc_stage_weights(*args, None) < 0 and b"stage_weights" in lib.cdc_last_error()
    # the fused launches: a weight without the fused loss's labels
    a = _lib.RowdotBwdArgs()
    a.n_groups, a.M, a.workspace, a.sigmoid = 1, 4, 16, 1
    a.g[0].dout = a.g[0].x = a.g[0].w = a.g[0].out = 16
    a.g[0].K = 4
    a.bce_weight = 16
    assert lib.cdc_rowdot_bwd(C.byref(a), None) == -1 and b"bce_weight" in lib.cdc_last_error()
    h = _lib.HeadArgs()
    h.n_tower, h.M, h.out, h.workspace, h.d_out = 1, 4, 16, 16, 16
    h.t[0].x = h.t[0].w = 16
    h.t[0].K = 4
    h.bce_weight = 16
    assert lib.cdc_head_bwd(C.byref(h), None) == -1 and b"bce_weight" in lib.cdc_last_error()
