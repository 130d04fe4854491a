"""tests/bn_ref.py held on the CPU: the float64 BatchNorm restatement against torch.nn.BatchNorm1d in float64 and the
reference's skip rules; every derived bound accepts the float64 result rounded once and an fp32 restatement in the kernels'
operation order, and rejects every seeded defect at every shape tests/test_gpu_batchnorm.py runs; no bound is looser than the
suite's figures; the dropout streams agree with a scalar Python restatement of csrc/common.h."""
import numpy as np
import pytest
import torch

import bn_ref as R
from helpers import OUT_FIG, SUM_FIG, assert_bounded


compare = R.compare


def _rounded(W):
    out = []
    for w in W:
        d = {k: v[0].astype(np.float32) for k, v in w.items() if isinstance(v, tuple)}
        for k in ("yh", "dxh"):
            if k in d:
                d[k] = R.bf16_round(d[k])
        out.append(d)
    return out


def _saved(s, D, K):
    """the backward's operands from an fp32 forward: y's buffer, save_mean, save_invstd (eval: from the running stats)"""
    full = lambda i, v: _scatter(s, i, v)
    Y = [full(i, k["y"] if "y" in k else k["yh"]) for i, k in enumerate(K)]
    if not s["training"]:
        return (Y,) + R.eval_saved(s, D)
    nan = lambda C: np.full(C, np.nan, np.float32)
    return Y, [k.get("save_mean", nan(C)) for k, C in zip(K, s["C"])], [k.get("save_invstd", nan(C)) for k, C in zip(K, s["C"])]


def _scatter(s, i, v):
    out = np.full((R.launch_rows(s), s["C"][i]), np.nan, np.float32)
    out[R.seg_rows(s, i)] = v
    return out


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("M", [2, 65, 130])
def test_reference_matches_torch_float64(training, M):
    s = R.spec("torch", (5, 9), M, relu=0, training=int(training))
    D = R.make_data(s)
    F = R.ref_forward(s, D)
    for i, C in enumerate(s["C"]):
        bn = torch.nn.BatchNorm1d(C, eps=float(np.float32(s["eps"])), momentum=float(np.float32(s["momentum"]))).double()
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(D["gamma"][i]))
            bn.bias.copy_(torch.from_numpy(D["beta"][i]))
            bn.running_mean.copy_(torch.from_numpy(D["rm"][i]))
            bn.running_var.copy_(torch.from_numpy(D["rv"][i]))
            bn.num_batches_tracked.fill_(D["nbt"][i])
        bn.train(training)
        x = torch.from_numpy(D["x"][i]).double().requires_grad_(True)
        y = bn(x)
        dy = torch.from_numpy(D["dy"][i]).double()
        (y * dy).sum().backward()
        close = lambda a, b: np.testing.assert_allclose(np.asarray(a), b.detach().numpy(), rtol=1e-10, atol=1e-12)
        close(F[i]["y"][0], y)
        close(F[i]["running_mean"][0], bn.running_mean)
        close(F[i]["running_var"][0], bn.running_var)
        assert F[i]["nbt"] == int(bn.num_batches_tracked)
        if training:
            mean, inv = F[i]["save_mean"][0], F[i]["save_invstd"][0]
        else:
            mean, inv = R.f64(D["rm"][i]), 1.0 / np.sqrt(R.f64(D["rv"][i]) + float(np.float32(s["eps"])))
        B = R.ref_backward(dict(s, C=(C,), pad=(3,), seg_group=(0,), acc=(0,)), {k: [v[i]] for k, v in D.items()}, [F[i]["y"][0]], [mean], [inv])[0]
        close(B["dx"][0], x.grad)
        close(B["dgamma"][0], bn.weight.grad)
        close(B["dbeta"][0], bn.bias.grad)


def test_reference_skip_rules():
    """model/layer.py's MultiLayerPerceptron and star.py's MDR_BatchNorm skip BatchNorm for exactly one row (skip_le1 = 0), its DNN
    for at most one (skip_le1 = 1): y = relu(x), statistics and num_batches_tracked untouched, gamma / beta ignored, dx = dz.
    An EMPTY batch that is not skipped (a domain absent from the batch under MDR_BatchNorm): torch counts the batch and leaves
    the running statistics alone."""
    for le1, M, skip in ((0, 1, True), (1, 1, True), (1, 0, True), (0, 0, False), (0, 2, False), (1, 2, False)):
        s = R.spec("skip", (5,), max(M, 1), groups=(M, 1 - M if M < 1 else 0), seg_group=(0,), skip_le1=le1)
        D = R.make_data(s)
        F = R.ref_forward(s, D)[0]
        assert F["written"] == (None if M == 0 and not skip else not skip) and F["nbt"] == D["nbt"][0] + (0 if skip else 1)
        rows = R.seg_rows(s, 0)
        if skip:
            assert np.array_equal(F["y"][0], np.maximum(R.f64(D["x"][0])[rows], 0)) and not F["y"][1].any()
            assert np.array_equal(F["running_mean"][0], D["rm"][0]) and np.array_equal(F["running_var"][0], D["rv"][0])
            if M:
                B = R.ref_backward(s, D, [F["y"][0]], [None], [None])[0]
                assert np.array_equal(B["dx"][0], np.where(F["y"][0] > 0, R.f64(D["dy"][0])[rows], 0.0))
                assert not B["dgamma"][0].any() and not B["dbeta"][0].any()
        if M == 0 and not skip:
            bn = torch.nn.BatchNorm1d(5).double()
            with torch.no_grad():
                bn.running_mean.copy_(torch.from_numpy(D["rm"][0]))
                bn.running_var.copy_(torch.from_numpy(D["rv"][0]))
                bn.num_batches_tracked.fill_(D["nbt"][0])
            assert bn(torch.zeros(0, 5, dtype=torch.float64)).shape == (0, 5)
            assert int(bn.num_batches_tracked) == F["nbt"]
            assert np.array_equal(bn.running_mean.numpy(), F["running_mean"][0]) and np.array_equal(bn.running_var.numpy(), F["running_var"][0])


def _masks_differ(s, D, Y):
    """mask_from_x changes something iff some element's x and y differ in sign; at a handful of elements they may all agree, from
    64 elements of a normalised group on they must not"""
    n, big = 0, False
    for i in range(len(s["C"])):
        rows = R.seg_rows(s, i)
        n += int(((D["x"][i][rows] > 0) != (Y[i][rows] > 0)).sum())
        big |= rows.size * s["C"][i] >= 64 and not R.skipped(s, rows.size, True)
    assert n or not big, f"{s['name']}: x and y agree in sign everywhere"
    return n > 0


def _applies(defect, s, backward, parts, D=None, Y=None):
    live = [len(R.seg_rows(s, i)) for i in range(len(s["C"]))]
    normed = [m for m in live if m >= 1 and not R.skipped(s, m, backward)]
    masked = bool(s["relu"]) or s["drop_p"] > 0
    return {"stats_drop_last_row": bool(s["training"]) and any(m >= 2 for m in normed),
            "drop_tile_tail": True,
            "biased_running_var": bool(s["training"]) and s["running"] and any(m >= 2 for m in normed),
            "launch_M": bool(s["training"]) and s["groups"] is not None and any(m >= 2 and m != R.launch_rows(s) for m in normed),
            "neighbour_gamma": s["gb"] and len(s["C"]) >= 2 and bool(normed),
            "acc_off": any(a and m for a, m in zip(s["acc"], live)),
            "mask_from_x": masked and defect == "mask_from_x" and _masks_differ(s, D, Y),
            "no_mask_scale": s["drop_p"] > 0,
            "one_row_rank": parts is not None and any(len(p) == 1 and m > 1 for pp, m in zip(parts, live) for p in pp)}[defect]


def _specs_with_parts():
    out = [(s, None) for s in R.geometry_specs() + R.group_specs() + R.flag_specs()]
    for name in R.DP_SPLITS:
        for pad in (3, 4):
            u, ranks, parts = R.dp_specs(name, pad)
            out.append((u, parts))
    return out


def test_bounds_accept_clean_and_reject_seeded_defects(monkeypatch):
    """At every spec the GPU tests launch (geometry, launch shapes, row groups, the flag table, the unions of the data-parallel
    splits): each bound accepts the float64 result rounded once (bf16 outputs: rounded to bf16) and the fp32 restatement in the
    kernels' order, is no looser than the suite's figure, and rejects each defect of bn_ref.FWD_DEFECTS / BWD_DEFECTS wherever the
    defect can change anything at that spec; every defect defined is seen at least once."""
    monkeypatch.delenv("CDC_RECORD_MARGINS", raising=False)
    seen = set()
    for s, parts in _specs_with_parts():
        what = f"{s['name']} M={s['M']}"
        D = R.make_data(s)
        F = R.ref_forward(s, D, n_ranks=2 if parts else 1)
        K = R.kernel_forward32(s, D)
        compare(_rounded(F), F, what + " rounded")
        compare(K, F, what + " fp32 order")
        Y, MEAN, INV = _saved(s, D, K)
        B = R.ref_backward(s, D, Y, MEAN, INV, parts=parts)
        compare(_rounded(B), B, what + " bwd rounded")
        if parts is None:
            compare(R.kernel_backward32(s, D, Y, MEAN, INV), B, what + " bwd fp32 order")
        else:
            U = R.ref_backward(s, D, Y, MEAN, INV)                              # the ranks' local sums add up to the group's
            for u, b in zip(U, B):
                for k in ("dgamma", "dbeta"):
                    tot = sum(b[f"{k}_r{r}"][0] for r in range(2))
                    assert_bounded(tot, u[k][0], sum(b[f"{k}_r{r}"][1] for r in range(2)) + 1e-300, what + " " + k)
                assert np.array_equal(u["dx"][0], b["dx"][0]) or np.allclose(u["dx"][0], b["dx"][0], rtol=1e-12, atol=1e-12)
        for W in (F, B):
            for w in W:
                for k, v in w.items():
                    if isinstance(v, tuple) and k not in ("pre", "yh", "dxh"):
                        fig = SUM_FIG if k.startswith(("dgamma", "dbeta")) else OUT_FIG
                        mag = np.maximum(np.abs(v[0]), w["terms"].get(k, 0.0))       # y, dx: at the terms' magnitude (bn_ref.py)
                        ok = np.isnan(v[0]) | (v[1] <= (fig[1] + fig[0] * mag) * (1 + 1e-12))
                        assert ok.all(), f"{what} {k}: looser than the suite's figure"
        for defect in R.FWD_DEFECTS:
            if _applies(defect, s, False, parts):
                seen.add(defect)
                with pytest.raises(AssertionError):
                    compare(_rounded(R.ref_forward(s, D, defect)), F, f"{what} {defect}")
        for defect in R.BWD_DEFECTS:
            if _applies(defect, s, True, parts, D, Y):
                seen.add(defect)
                with pytest.raises(AssertionError):
                    compare(_rounded(R.ref_backward(s, D, Y, MEAN, INV, defect, parts=parts)), B, f"{what} bwd {defect}")
    assert seen == set(R.FWD_DEFECTS + R.BWD_DEFECTS), seen


def test_offset_case_cancellation_term_is_below_the_figure():
    """|mean| / std = 10^3: the cancellation term of the invstd bound is still far below OUT_FIG, and the ratio at which it
    passes the figure is the accuracy limit DESIGN.md states for the one-pass variance."""
    s = [t for t in R.flag_specs() if t["data"] == "offset" and t["M"] == 577][0]
    D = R.make_data(s)
    F = R.ref_forward(s, D)
    for i, f in enumerate(F):
        x = R.f64(D["x"][i])
        ratio = np.abs(x.mean(0)) / x.std(0)
        assert (ratio > 500).all() and (ratio < 2000).all()
        inv = f["save_invstd"][0]
        assert (f["dinv_raw"] <= 0.02 * (OUT_FIG[1] + OUT_FIG[0] * inv)).all()
    assert 1.0e4 < R.one_pass_limit(577) < 1.0e5


def test_dropout_streams_against_scalar_restatement():
    M64, M32 = (1 << 64) - 1, (1 << 32) - 1

    def uniform(seed, idx):
        z = (seed + idx * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        return np.float32(z >> 40) * np.float32(1.0 / 16777216.0)

    def h32(x):
        x &= M32
        x ^= x >> 16
        x = (x * 0x7feb352d) & M32
        x ^= x >> 15
        x = (x * 0x846ca68b) & M32
        return x ^ (x >> 16)

    seed, p, C, seg = R.SEED, 0.25, 6, 5
    rows = np.array([0, 1, 77, 40000])
    for step in (None, 3, 70000):
        sd = seed if step is None else (seed + step * 0xD1342543DE82EF95) & M64
        want = np.array([[not (uniform(sd, ((seg + 64) << 56) ^ (int(r) * C + c)) < np.float32(p)) for c in range(C)] for r in rows])
        assert np.array_equal(R.keep_mask_uniform(seed, step, seg, rows, C, p), want)
        s32 = ((seed & M32) ^ (((seed >> 32) * 0x9E3779B1) & M32))
        if step is not None:
            s32 ^= (step * 0x85EBCA77) & M32
        s32 = h32(s32 + (64 + seg) * 0xC2B2AE3D)
        want = np.zeros((len(rows), C), bool)
        for a, r in enumerate(rows):
            for c in range(C):
                h = h32(s32 + int(r) * 0x9E3779B1 + (c >> 1) * 0x85EBCA77)
                want[a, c] = ((h >> 16) if c & 1 else (h & 0xFFFF)) >= 16384
        assert np.array_equal(R.keep_mask_bits16(seed, step, seg, rows, C, p), want)
    keep = R.keep_mask_bits16(seed, 1, 0, np.arange(4096), 64, p)
    assert abs(keep.mean() - 0.75) < 0.01 and abs(R.keep_mask_uniform(seed, 1, 0, np.arange(4096), 64, p).mean() - 0.75) < 0.01
