"""CDC's batched probe evaluation: the segment-BCE launch `cdc_eval_segments` against float64,
`evaluate.eval_segments` in both metrics, `probe.ProbeEval` against the per-domain forward it replaces, and
`CDCTrainer(batched_probe=True)` against the per-domain loop from identical seeds."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import assert_close, make_ids

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SIZES = [0, 1, 2, 63, 64, 65, 257, 1000]
PAD = 100


def _bce64(p, t):
    """the step's per-element BCE (ATen's) in float64 on the given probabilities"""
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (t - 1.0) * np.maximum(np.log1p(-p), -100.0) - t * np.maximum(np.log(p), -100.0)


def _seg_means(vals, sizes):
    out, lo = [], 0
    for s in sizes:
        out.append(float(np.mean(vals[lo:lo + s])) if s else float("nan"))
        lo += s
    return np.array(out)


def _segments_raw(dev, probs, ld, label, sizes, cols, want_rows=True):
    """cdc_eval_segments through the C-ABI: -> (loss f64 [n_seg], sel_pred, seg_of_row, err) with the two row outputs pre-filled
    with sentinels"""
    from cdcmdr_amd import _lib
    lib = _lib.load()
    rows = label.numel()
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d_start = torch.from_numpy(starts).to(dev)
    d_col = torch.from_numpy(np.asarray(cols, dtype=np.int32)).to(dev)
    loss = torch.full((len(sizes),), -7.0, dtype=torch.float64, device=dev)
    sel = torch.full((rows,), -3.0, dtype=torch.float32, device=dev)
    seg = torch.full((rows,), -5, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = lib.cdc_eval_segments(probs.data_ptr(), ld, label.data_ptr(), d_start.data_ptr(), len(sizes), d_col.data_ptr(), loss.data_ptr(),
                               sel.data_ptr() if want_rows else None, seg.data_ptr() if want_rows else None, err.data_ptr(), rows,
                               probs.shape[1], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.cdc_last_error()
    return loss, sel, seg, err


def _kernel_case(n_cols, seed):
    """host arrays: probs [rows, ld] (padding rows NaN), labels (padding 7), columns, the selected probability of every row"""
    rng = np.random.default_rng(seed)
    ld = n_cols + 3
    n = sum(SIZES)
    rows = n + PAD
    probs = (1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal((rows, ld))))).astype(np.float32)
    probs = np.clip(probs, np.float32(1e-30), np.float32(1.0 - 2.0 ** -24))
    label = rng.integers(0, 2, size=rows).astype(np.int16)
    cols = rng.integers(0, n_cols, size=len(SIZES))
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    label[starts[5]:starts[6]] = 0                                   # one segment all-zero labels, one all-one
    label[starts[6]:starts[7]] = 1
    plants = [np.float32(0.0), np.float32(1.0), np.float32(1.0 - 2.0 ** -24)]
    for k, (p, t) in enumerate([(p, t) for p in plants for t in (0, 1)]):       # both -100 clamps, under both labels
        r = starts[7] + 11 + 37 * k
        probs[r, cols[7]], label[r] = p, t
    probs[starts[3] + 5, cols[3]], label[starts[3] + 5] = 0.0, 1     # and in a segment that is not a multiple of the wave
    probs[starts[6] + 200, cols[6]] = 1.0                            # label 1: log(1) = 0
    probs[starts[5] + 64, cols[5]] = 1.0                             # label 0: the clamp, in the last row of a 65-row segment
    probs[n:] = np.nan
    label[n:] = 7
    seg_of = np.repeat(np.arange(len(SIZES)), SIZES)
    sel = probs[np.arange(n), cols[seg_of]]
    return probs, ld, label, cols, sel, seg_of


@pytest.mark.parametrize("n_cols", [1, 3, 5])
def test_segment_bce_against_float64(cuda, n_cols):
    from cdcmdr_amd.evaluate import eval_segments
    probs, ld, label, cols, sel, seg_of = _kernel_case(n_cols, 10 + n_cols)
    n = sum(SIZES)
    want = _seg_means(_bce64(sel, label[:n]), SIZES)
    d_probs = torch.from_numpy(probs).to(cuda)[:, :n_cols]           # a row-strided view: ld = n_cols + 3
    d_label = torch.from_numpy(label).to(cuda)
    loss, d_sel, d_seg, err = _segments_raw(cuda, d_probs, ld, d_label, SIZES, cols)
    got = loss.cpu().numpy()
    print("segment sizes", SIZES, "columns", cols.tolist())
    for s in range(len(SIZES)):
        print(f"  seg {s}: got {got[s]!r} want {want[s]!r} |d| {abs(got[s] - want[s]):.3e} allowed {4 * U * want[s] + 1e-12:.3e}")
    assert np.isnan(got[0]) and np.isnan(want[0])                    # the empty segment: torch's mean of nothing
    assert np.all(np.abs(got[1:] - want[1:]) <= 4 * U * want[1:] + 1e-12)
    assert float(want.max(initial=0, where=~np.isnan(want))) > 1.0 and np.any(_bce64(sel, label[:n]) == 100.0)
    assert int(err.item()) == 0, "padding rows must not trip the error word"
    assert np.array_equal(d_sel[:n].cpu().numpy().view(np.int32), sel.view(np.int32))
    assert np.array_equal(d_seg[:n].cpu().numpy(), seg_of.astype(np.int32))
    assert bool((d_sel[n:] == -3.0).all()) and bool((d_seg[n:] == -5).all()), "padding rows were written"
    loss2, d_sel2, d_seg2, _ = _segments_raw(cuda, d_probs, ld, d_label, SIZES, cols)
    assert np.array_equal(loss2.cpu().numpy().view(np.int64), got.view(np.int64)), "two calls, different bits"
    assert torch.equal(d_sel2, d_sel) and torch.equal(d_seg2, d_seg)
    # without the optional row outputs, and through the Python entry point: the same figures as float32, nothing read back
    loss3 = _segments_raw(cuda, d_probs, ld, d_label, SIZES, cols, want_rows=False)[0]
    assert np.array_equal(loss3.cpu().numpy().view(np.int64), got.view(np.int64))
    out = eval_segments(d_probs, d_label, SIZES, cols)
    assert out.dtype == torch.float32 and out.is_cuda and out.shape == (len(SIZES),)
    assert np.array_equal(out.cpu().numpy().view(np.int32), got.astype(np.float32).view(np.int32))
    assert int(eval_segments.last_err.item()) == 0
    if n_cols == 1:                                                  # seg_col=None scores every segment by column 0
        out0 = eval_segments(d_probs, d_label, SIZES)
        assert np.array_equal(out0.cpu().numpy().view(np.int32), out.cpu().numpy().view(np.int32))


def test_error_word_names_a_bad_row_inside_a_segment_only(cuda):
    from cdcmdr_amd.evaluate import eval_segments
    rng = np.random.default_rng(3)
    sizes, cols = [5, 0, 70, 300], [2, 0, 1, 0]
    n, rows = sum(sizes), sum(sizes) + 20
    base = rng.uniform(0.05, 0.95, size=(rows, 3)).astype(np.float32)
    label = rng.integers(0, 2, size=rows).astype(np.int16)

    def flag(probs, lab, metric="loss"):
        eval_segments(torch.from_numpy(probs).to(cuda), torch.from_numpy(lab).to(cuda), sizes, cols, metric)
        return int(eval_segments.last_err.item())

    assert flag(base, label) == 0
    p = base.copy()
    p[40, 1] = np.nan                                                # row 40 lies in segment 2, scored by column 1
    assert flag(p, label) == 41
    assert flag(p, label, "auc") == 41
    p = base.copy()
    p[40, 0] = p[40, 2] = np.nan                                     # a NaN in a column the segment is not scored by
    assert flag(p, label) == 0
    lab = label.copy()
    lab[200] = 2
    assert flag(base, lab) == 201
    p, lab = base.copy(), label.copy()
    p[n:] = np.nan                                                   # the same values in padding rows
    lab[n:] = 2
    assert flag(p, lab) == 0


def test_auc_mode_equals_eval_metrics_per_segment(cuda):
    from cdcmdr_amd.evaluate import eval_metrics, eval_segments
    rng = np.random.default_rng(5)
    sizes, cols = [1, 2, 65, 300], [1, 2, 0, 2]
    n, rows, ld = sum(sizes), sum(sizes) + 30, 5
    probs = (rng.integers(1, 8, size=(rows, ld)) / 8.0).astype(np.float32)       # eight distinct scores: ties everywhere
    label = rng.integers(0, 2, size=rows).astype(np.int16)
    label[1:3] = 1                                                   # a single-class segment (the one-row segment is one as well)
    probs[n:] = np.nan
    label[n:] = 7
    d_probs = torch.from_numpy(probs).to(cuda)[:, :3]
    d_label = torch.from_numpy(label).to(cuda)
    got = eval_segments(d_probs, d_label, sizes, cols, metric="auc")
    assert got.dtype == torch.float32 and got.shape == (4,)
    assert int(eval_segments.last_err.item()) == 0
    want, lo = [], 0
    for s, c in zip(sizes, cols):
        want.append(eval_metrics(d_probs[lo:lo + s, c].contiguous(), d_label[lo:lo + s])[0][-1].to(torch.float32))
        lo += s
    want = torch.stack(want)
    g, w = got.cpu().numpy(), want.cpu().numpy()
    print("auc per segment", g, "per-segment eval_metrics", w)
    assert np.isnan(w[0]) and np.isnan(w[1]) and not np.isnan(w[2]) and not np.isnan(w[3])
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[2:].view(np.int32), w[2:].view(np.int32))
    # an empty segment gives NaN as well
    got0 = eval_segments(d_probs, d_label, [0] + sizes, [0] + cols, metric="auc").cpu().numpy()
    assert np.isnan(got0[0]) and np.array_equal(got0[3:].view(np.int32), w[2:].view(np.int32))


# ---- ProbeEval against the per-domain forward ---------------------------------------------------------------------------
N_DOMAIN, N_CLUSTER, DOMAIN_IDX, BS = 6, 2, 4, 64
FD = [7, 300, 3, 50, N_DOMAIN, 29]


def _cdc_fixture(cuda, base, table_mode="lazy", n_causal_mask=3, dropout=0.2, batched_probe=False, **opt_kw):
    """the fixture of tests/test_gpu_cdc.py's loop tests"""
    from cdcmdr_amd.cdc_trainer import CDCTrainer
    from cdcmdr_amd.data import make_domain_loaders
    from cdcmdr_amd.model.cdc import CDC
    from cdcmdr_amd.optim import FusedAdam
    rng = np.random.default_rng(0)
    n = 1500
    X = torch.from_numpy(make_ids(rng, n, FD))
    y = torch.from_numpy(rng.integers(0, 2, size=(n, 1)).astype(np.int16))
    np.random.seed(1)
    torch.manual_seed(1)
    loaders, seq, w = make_domain_loaders(X, y, BS, cuda, DOMAIN_IDX, N_DOMAIN)
    cfg = types.SimpleNamespace(mmoe_n_expert=3, ple_n_expert_specific=2, ple_n_expert_shared=2, dataset_name="t", p_weight=0.5,
                                p_weight_method="linear_decay", p_weight_exp_decay=0.9, old_matrix_weight=0.3, affinity_func="minus",
                                use_atten=False)
    expert_dims = (16, 8) if base == "mmoe" else ((32, 16), (8,))
    cdc = CDC(FD, 4, N_CLUSTER, N_DOMAIN, base, expert_dims, (8,), DOMAIN_IDX, domain_cnt_weight=w, n_causal_mask=n_causal_mask,
              use_metric="loss", device=cuda, dropout=dropout, config=cfg).to(cuda).set_precision("f32")
    opt = FusedAdam(cdc.base_model_instance, table_mode=table_mode, **opt_kw)
    tr = CDCTrainer(cdc, opt, BS, loaders, N_DOMAIN, w, seq, warmup_step=1, update_matrix_step=1, update_interval=0,
                    batched_probe=batched_probe)
    return cdc, opt, tr


def _ragged_batches(tr, ragged=(1, 3)):
    """one batch per domain; for the domains of `ragged` the loader's short last batch"""
    batches = []
    for d in range(N_DOMAIN):
        X, y = tr.get_domain_data(d)
        for _ in range(8):
            if d not in ragged or X.shape[0] != BS:
                break
            X, y = tr.get_domain_data(d)
        batches.append((X, y))
    return batches


def _class_bound(p, t, rtol, atol):
    """what a deviation of every probability by rtol * p + atol can move the mean BCE by (the loss is monotone in p)"""
    p = np.asarray(p, dtype=np.float64)
    d = rtol * np.abs(p) + atol
    l0 = _bce64(p, t)
    return float(np.mean(np.maximum(np.abs(_bce64(np.clip(p + d, 0, 1), t) - l0), np.abs(_bce64(np.clip(p - d, 0, 1), t) - l0))))


def _eval_plans(base):
    """batch sizes of the base model's resident eval-mode forward plans"""
    return sorted(key[1] for key in base._cache().plans if key[0][0] == "fwd" and key[2] is False)


@pytest.mark.parametrize("base_name", ["mmoe", "ple"])
def test_probe_eval_matches_the_per_domain_forward(cuda, tmp_path, monkeypatch, base_name):
    from cdcmdr_amd.probe import ROWS_CAP, ProbeEval, pack_passes
    monkeypatch.chdir(tmp_path)
    cdc, opt, tr = _cdc_fixture(cuda, base_name)
    base = cdc.base_model_instance
    for _ in range(3):
        Xb, yb = tr.get_domain_data(0)
        tr._step(Xb, yb, "split", domain_i=0)
    opt.flush_table()
    torch.manual_seed(7)
    for m in base.modules():
        if getattr(m, "running_mean", None) is not None:
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    batches = _ragged_batches(tr)
    sizes = [int(X.shape[0]) for X, _ in batches]
    assert min(sizes) < BS == max(sizes)
    cols = [1, 0, 0, 1, 1, 0]
    base._cache().clear()
    results = {}
    for cap in (128, ROWS_CAP):
        pe = ProbeEval(base, N_CLUSTER, rows_cap=cap)
        base.train()
        loss = pe.run(batches, cols, "loss")
        assert base.training, "the module flag must be restored"
        base.eval()
        loss_again = pe.run(batches, cols, "loss")
        assert not base.training
        assert loss.dtype == torch.float32 and loss.shape == (N_DOMAIN,) and torch.equal(loss, loss_again)
        assert int(pe.last_err.item()) == 0
        want_B = 128 if cap == 128 else -(-sum(sizes) // 64) * 64
        assert pe.B == want_B
        assert _eval_plans(base).count(pe.B) == 1, "one eval plan for the probe size, not one per pass"
        auc = pe.run(batches, cols, "auc")
        # the forward the passes ran, staged again the same way at the same plan size: ProbeEval's own staging is held to it by
        # its losses at the kernel's bound (a misplaced row or a wrong tail would move a loss far beyond that)
        sel, passes = [], pack_passes(sizes, max(min(pe.B, cap), max(sizes)))
        assert len(passes) == (3 if cap == 128 else 1)
        with torch.no_grad():
            for first, last in passes:
                Xp = torch.cat([X for X, _ in batches[first:last]])
                out = base(torch.cat([Xp, Xp[:1].expand(pe.B - Xp.shape[0], -1)]))
                assert out.shape == (pe.B, N_CLUSTER)
                lo = 0
                for d in range(first, last):
                    sel.append(out[lo:lo + sizes[d], cols[d]].clone())
                    lo += sizes[d]
        for d, (_, y) in enumerate(batches):
            want = float(np.mean(_bce64(sel[d].cpu().numpy(), y.reshape(-1).cpu().numpy())))
            assert abs(float(loss[d]) - want) <= 4 * U * want + 1e-12 + 2.0 ** -24 * want, f"cap {cap} domain {d}: staging"
        results[cap] = (loss.cpu().numpy(), auc.cpu().numpy(), sel)
    assert _eval_plans(base) == sorted({128, -(-sum(sizes) // 64) * 64}), "the probe sizes only: nothing per pass or per batch"
    # the per-domain forward the batched pass replaces
    from cdcmdr_amd.evaluate import eval_metrics
    base.eval()
    bit_equal = True
    with torch.no_grad():
        for d, (X, y) in enumerate(batches):
            p_d = base(X)[:, cols[d]]
            t = y.reshape(-1).cpu().numpy()
            p64 = p_d.cpu().numpy().astype(np.float64)
            want = float(np.mean(_bce64(p64, t)))
            allowed = 4 * U * want + 1e-12 + _class_bound(p64, t, 2e-5, 2e-6)
            want_auc = float(eval_metrics(p_d.contiguous(), y.reshape(-1))[0][-1])
            for cap, (loss, auc, sel) in results.items():
                assert_close(sel[d], p_d, 2e-5, 2e-6, f"{base_name} cap {cap} domain {d}: selected probabilities")
                same = torch.equal(sel[d], p_d)
                bit_equal = bit_equal and same
                print(f"{base_name} cap {cap} domain {d} ({sizes[d]} rows, tower {cols[d]}): loss {loss[d]!r} want {want!r} "
                      f"|d| {abs(loss[d] - want):.3e} allowed {allowed:.3e}; probabilities bit-equal: {same}; "
                      f"max |dp| {float((sel[d] - p_d).abs().max()):.3e}; auc {auc[d]!r} want {want_auc!r}")
                # the float32 the result is returned as adds half an ulp of it
                assert abs(float(loss[d]) - want) <= allowed + 2.0 ** -24 * want
                if same:                                             # the rank sums are integers: only the float32 it is returned as
                    assert abs(float(auc[d]) - want_auc) <= 2.0 ** -24
    print(f"{base_name}: batched and per-domain probabilities bit-equal on every domain: {bit_equal}")


def test_probe_eval_bf16_ple_at_the_reference_widths(cuda):
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.probe import ProbeEval
    fd = [7, 300, 3, 50, 3, 29]
    torch.manual_seed(11)
    model = PLE(fd, 16, 3, 2, 2, ((256, 128), (64,)), (64, 32), dropout=0.2).to(cuda).set_precision("bf16")
    for m in model.modules():
        if getattr(m, "running_mean", None) is not None:
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    rng = np.random.default_rng(4)
    sizes, cols = [64, 64, 37], [2, 0, 1]
    batches = [(torch.from_numpy(make_ids(rng, b, fd)).to(cuda), torch.from_numpy(rng.integers(0, 2, size=(b, 1)).astype(np.int16)).to(cuda))
               for b in sizes]
    model.train()
    pe = ProbeEval(model, 3)
    loss = pe.run(batches, cols, "loss").cpu().numpy()
    assert model.training and pe.B == 192
    model.eval()
    with torch.no_grad():
        staged = torch.cat([X for X, _ in batches] + [batches[0][0][:1].expand(pe.B - sum(sizes), -1)])
        out = model(staged)
        lo = 0
        for d, (X, y) in enumerate(batches):
            p_d = model(X)[:, cols[d]]
            assert_close(out[lo:lo + sizes[d], cols[d]], p_d, 5e-3, 2e-3, f"bf16 domain {d}: selected probabilities")
            t = y.reshape(-1).cpu().numpy()
            # ProbeEval's own staging against this one, at the kernel's bound: the same plan scored the same rows
            staged_want = float(np.mean(_bce64(out[lo:lo + sizes[d], cols[d]].cpu().numpy(), t)))
            assert abs(float(loss[d]) - staged_want) <= 4 * U * staged_want + 1e-12 + 2.0 ** -24 * staged_want, f"bf16 domain {d}: staging"
            p64 = p_d.cpu().numpy().astype(np.float64)
            want = float(np.mean(_bce64(p64, t)))
            allowed = 4 * U * want + 1e-12 + _class_bound(p64, t, 5e-3, 2e-3) + 2.0 ** -24 * want
            print(f"bf16 domain {d}: loss {loss[d]!r} want {want!r} |d| {abs(loss[d] - want):.3e} allowed {allowed:.3e}; "
                  f"max |dp| {float((out[lo:lo + sizes[d], cols[d]] - p_d).abs().max()):.3e}")
            assert abs(float(loss[d]) - want) <= allowed
            lo += sizes[d]


def test_update_matrix_batched_probe_equals_the_per_domain_loop(cuda, tmp_path, monkeypatch):
    """The probes' training steps do not depend on the evaluation: with the same draws (every domain's loader once per
    evaluation, in order, no extra random numbers) the optimiser state after update_matrix() is bit-equal between the two
    modes, and the matrices agree to the fp32 parity class."""
    monkeypatch.chdir(tmp_path)
    res = {}
    for batched in (False, True):
        cdc, opt, tr = _cdc_fixture(cuda, "mmoe", table_mode="lazy", n_causal_mask=2, dropout=0.0, batched_probe=batched,
                                    fast_replay=False, flush_every=4)
        tr.warmup_step, tr.update_matrix_step = 3, 2
        for _ in range(3):
            Xb, yb = tr.get_domain_data(0)
            tr._step(Xb, yb, "split", domain_i=0)
        groups = tr.update_matrix()
        opt.flush_table()
        base = cdc.base_model_instance
        res[batched] = {"mask": cdc.matrix_mask.cpu().clone(), "A": cdc.matrix_A.cpu().clone(), "B": cdc.matrix_B.cpu().clone(),
                        "m": opt.table_m.cpu().clone(), "v": opt.table_v.cpu().clone(), "step": int(opt.step_dev.item()),
                        "last": opt.table_last.cpu().clone(),
                        "sd": {k: v.detach().cpu().clone() for k, v in base.state_dict().items()}, "groups": list(groups)}
        print(f"batched_probe={batched}: domain2group_list {list(groups)}")
    a, b = res[False], res[True]
    for name in ("mask", "A", "B"):
        assert bool(torch.isfinite(torch.as_tensor(b[name])).all())
        assert_close(b[name], a[name], 2e-5, 2e-6, f"matrix_{name}")
        print(f"matrix_{name}: max |d| {float((b[name] - a[name]).abs().max()):.3e}, bit-equal {torch.equal(a[name], b[name])}")
    assert a["step"] == b["step"] > 3
    assert torch.equal(a["last"], b["last"])
    assert torch.equal(a["m"], b["m"]), "exp_avg of the table differs"
    assert torch.equal(a["v"], b["v"]), "exp_avg_sq of the table differs"
    assert set(a["sd"]) == set(b["sd"])
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), f"{k} differs between the two modes"
