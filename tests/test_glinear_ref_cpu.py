"""tests/glinear_ref.py held on the CPU: the float64 restatement of the grouped linear launches against torch in float64; at every
launch tests/test_gpu_glinear.py runs, every derived bound accepts the float64 result rounded once, is nowhere looser than the
suite's present figures, and rejects each seeded defect; the slices are those of the kernels' own arithmetic; the forward's
dropout stream keeps 1 - p of the elements."""
import numpy as np
import pytest
import torch

import glinear_ref as R
from helpers import assert_bounded

RUNS = R.all_ref_runs()
FIG = {"y": R.Y_FIG, "d": R.G_FIG, "s": R.G_FIG}


def _rounded(W):
    return {k: v[0].astype(np.float32) for k, v in W.items()}


def _violates(got, W):
    for k, (want, bound) in W.items():
        if k not in got or got[k].shape != want.shape or not (np.abs(R.f64(got[k]) - want) <= bound).all():
            return True
    return False


def test_reference_matches_torch_float64():
    t = lambda a: torch.from_numpy(R.f64(a))
    c = R.fwd_case("torch_f", 40, 65, [5, 9], act=[3, 0])
    D = R.make_data(c)
    W = R.ref_fwd(c, D, R.F32)
    for g, N in enumerate(c["Ns"]):
        y = torch.nn.functional.linear(t(D["x"]), t(D["w"][g]), t(D["b"][g]))
        y[:, :c["act"][g]] = torch.relu(y[:, :c["act"][g]])
        np.testing.assert_allclose(W[f"y{g}"][0], y.numpy(), rtol=1e-12, atol=1e-13)
    c = R.bwdx_case("torch_x", 33, [(7, 5, 1)], [(9, 0), (4, 0)], mask_scale=1.25)
    D = R.make_data(c)
    want = sum(t(D["dz"][s]) @ t(D["w"][s]) for s in range(2))
    want[:, :5] = torch.where(t(D["mask"][0])[:, :5] > 0, want[:, :5] * 1.25, torch.zeros(()).double())
    np.testing.assert_allclose(R.ref_bwdx(c, D, R.F32)["dx0"][0], (want + t(D["dx0"][0])).numpy(), rtol=1e-12, atol=1e-13)
    c = R.bwdw_case("torch_w", [(100, 6, 11, 1, 1, 0)], split=3)
    D = R.make_data(c)
    x, w = t(D["x"][0]), torch.zeros(6, 11, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.linear(x, w, b) * t(D["dz"][0])).sum().backward()
    W = R.ref_bwdw(c, D, R.F32, 32)
    np.testing.assert_allclose(W["dw0"][0], (w.grad + t(D["dw0"][0])).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(W["db0"][0], (b.grad + t(D["db0"][0])).numpy(), rtol=1e-12, atol=1e-12)
    # bf16: the operands are rounded, the contraction is not
    W = R.ref_fwd(R.fwd_case("torch_f", 40, 65, [5, 9], act=[0, 0], bias=False), R.make_data(R.fwd_case("torch_f", 40, 65, [5, 9])), R.BF16)
    D = R.make_data(R.fwd_case("torch_f", 40, 65, [5, 9]))
    np.testing.assert_allclose(W["y0"][0], R.f64(R.bf16_round(D["x"])) @ R.f64(R.bf16_round(D["w"][0])).T, rtol=1e-12, atol=1e-13)


def test_slices_restate_the_kernels_arithmetic():
    """chunk = ceil(ceil(M / S) / unit) unit, at least one unit: whole slices first, one partial, the rest empty; together the rows"""
    for unit in (32, 64):
        for M in (0, 1, 31, 64, 65, 200, 1000):
            for S in (1, 2, 3, 5, 8, 9):
                sl = R.slices(M, S, unit)
                chunk = max(((M + S - 1) // S + unit - 1) // unit * unit, unit)
                assert len(sl) == S and sum(rn for _, rn in sl) == M
                for s, (r0, rn) in enumerate(sl):
                    assert rn == max(min(M - s * chunk, chunk), 0) and (rn == 0 or r0 == s * chunk)
    assert [rn for _, rn in R.slices(65, 8, 32)] == [32, 32, 1, 0, 0, 0, 0, 0]
    assert [rn for _, rn in R.slices(65, 8, 64)] == [64, 1, 0, 0, 0, 0, 0, 0]


def test_slab_layout_is_the_documented_one():
    c = R.bwdw_case("layout", [(10, 3, 5, 1, 0, 0), (10, 2, 7, 0, 0, 0), (10, 4, 1, 1, 0, 0)], split=2, defer=1)
    off, stride = R.slab_layout(c)
    assert off == [(0, 15), (18, 32), (34, 38)] and stride == 42


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[f"{t}-{c['name']}-{'bf16' if p == R.BF16 else 'f32'}" for t, c, p, _ in RUNS])
def test_bounds_accept_the_rounded_reference_and_keep_the_figures(i):
    tag, c, prec, kw = RUNS[i]
    D = R.make_data(c)
    W = R.ref(tag, c, D, prec, **kw)
    assert W, "nothing to compare"
    for k, (want, bound) in W.items():
        assert_bounded(want.astype(np.float32), want, bound, f"{c['name']} {k}")
        rtol, atol = FIG[k[0]]
        assert (bound <= atol + rtol * np.abs(want)).all() and (bound >= 0).all(), f"{c['name']} {k}: looser than the present figure"
        live = np.abs(want) > 0
        assert (bound[live] > 0).all(), f"{c['name']} {k}: a zero bound on a nonzero value"


def test_bounds_reject_seeded_defects():
    seen = {d: 0 for d in R.DEFECTS}
    for tag, c, prec, kw in RUNS:
        D = R.make_data(c)
        W = R.ref(tag, c, D, prec, **kw)
        assert not _violates(_rounded(W), W)
        for d in R.DEFECTS:
            if d == "slab_db_after_next_dw":
                if not (tag == "bwdw" and c["defer"]):
                    continue
                want, bound = R.slab_sums(c, W, W)
                got = R.slab_sums(c, W, W, defect=d)[0].astype(np.float32)
                ok = np.isfinite(want)
                if np.array_equal(got[ok], want[ok].astype(np.float32)):
                    continue
                assert not (np.abs(R.f64(got) - want)[ok] <= bound[ok]).all(), f"{c['name']}: {d} passes the bounds"
                seen[d] += 1
                continue
            if (d in ("db_kind", "operand_unrounded") and prec != R.BF16) or (d == "ragged_off" and c["rows"] is None):
                continue
            B = _rounded(R.ref(tag, c, D, prec, defect=d, **kw))
            if all(np.array_equal(B[k], W[k][0].astype(np.float32)) for k in W):
                continue                                           # the defect changes nothing at this launch
            assert _violates(B, W), f"{c['name']} ({'bf16' if prec == R.BF16 else 'f32'}): {d} passes the bounds"
            seen[d] += 1
    assert all(seen.values()), f"defects never applied: {[d for d, n in seen.items() if not n]}"
    print("defects seen:", seen)


def test_a_defect_applies_wherever_its_path_is_taken():
    """the filter above (`changes nothing`) must not hide a defect: at these launches each one has to change the result"""
    must = {"k_tail": ("fwd", "bwdx", "bwdw"), "no_bias": ("fwd",), "relu_extra_col": ("fwd",), "seg_omitted": ("bwdx",),
            "mask_extra_col": ("bwdx",), "no_mask_scale": ("bwdx",), "acc_off": ("bwdx", "bwdw"), "slice_last_row": ("bwdw",),
            "slice_twice": ("bwdw",), "ragged_off": ("fwd", "bwdx", "bwdw"), "db_kind": ("bwdw",), "operand_unrounded": ("fwd", "bwdx", "bwdw")}
    hit = {(d, t): 0 for d, ts in must.items() for t in ts}
    for tag, c, prec, kw in RUNS:
        D = R.make_data(c)
        W = R.ref(tag, c, D, prec, **kw)
        for d, ts in must.items():
            if tag in ts and not (d in ("db_kind", "operand_unrounded") and prec != R.BF16) and not (d == "ragged_off" and c["rows"] is None):
                B = _rounded(R.ref(tag, c, D, prec, defect=d, **kw))
                hit[(d, tag)] += int(any(not np.array_equal(B[k], W[k][0].astype(np.float32)) for k in W))
    assert all(n >= 2 for n in hit.values()), {k: n for k, n in hit.items() if n < 2}


def test_dropout_stream_keeps_one_minus_p():
    n_cases = 0
    for c in R.fwd_cases():
        if c["p"] <= 0:
            continue
        kept, total = 0, 0
        for g, N in enumerate(c["Ns"]):
            lo, Mg = R.group_rows(c, g)
            k = R.fwd_keep(c, g, lo, Mg)[:, :c["act"][g]]
            kept, total = kept + int(k.sum()), total + k.size
        assert total >= 1000, f"{c['name']}: too few elements to test the rate"
        sigma = np.sqrt(total * c["p"] * (1 - c["p"]))
        assert abs(kept - total * (1 - c["p"])) <= 4 * sigma, f"{c['name']}: kept {kept} of {total}"
        n_cases += 1
    assert n_cases >= 2
    # the step moves the stream; another group's stream differs
    a = R.keep_mask_uniform(R.SEED, None, 0 - 64, np.arange(64), 64, 0.2)
    assert (a != R.keep_mask_uniform(R.SEED, 1, 0 - 64, np.arange(64), 64, 0.2)).any()
    assert (a != R.keep_mask_uniform(R.SEED, None, 1 - 64, np.arange(64), 64, 0.2)).any()
