"""tests/gemm2_ref.py held on the CPU: the float64 restatement of cdc_gemm_bf16_nt against torch in float64 (F.linear, autograd
for the grad-input); at every launch tests/test_gpu_gemm2_direct.py runs, every derived bound accepts the float64 result rounded
once (yh once more to bf16), is nowhere looser than the suite's present figures, and rejects each seeded defect; the 16-bit
dropout stream keeps 1 - p of the elements and moves with the stream id and the step; the launcher's tile choice restated puts the
four automatic launches in the four branches; the argument blocks of the GPU cases are well formed."""
import numpy as np
import pytest
import torch

import gemm2_ref as R
from glinear_ref import G_FIG, Y_FIG

CASES = R.all_cases()
IDS = [c["name"] for c in CASES]


def _passes(c, got, W):
    try:
        R.check(c, got, W, c["name"])
    except AssertionError:
        return False
    return True


def _same(A, B):
    return A.keys() == B.keys() and all(np.array_equal(A[k], B[k], equal_nan=True) for k in A)


def test_case_names_are_unique_and_cover_the_issue():
    assert len(set(IDS)) == len(IDS)
    assert {c["outs"][0]["M"] for c in R.geometry_cases()} == set(R.GEO_M)
    for c in R.geometry_cases():
        assert {(O["N"], O["act"]) for O in c["outs"]} == {(N, a) for N in R.GEO_N for a in (0, N, 36)}
    assert [R.slab_counts(R.ring_case(), o) for o in range(6)] == [[1], [2], [3], [4], [5], [7]]
    s1, s3, s32, s5 = R.segment_cases()
    assert R.slab_counts(s3, 0) == [1, 2, 1] and R.slab_counts(s5, 0) == [1] * 5 and len(s32["segs"]) == 32 and len(s32["outs"]) == 3
    assert [o for _, o, _ in s32["segs"]] == [s % 3 for s in range(32)], "interleaved in launch order"
    # a segment change falls on every ring position, at every depth
    for depth in (2, 3, 4):
        pos = set()
        for o in range(3):
            pos |= {int(x) % depth for x in np.cumsum(R.slab_counts(s32, o))[:-1]}
        assert pos == set(range(depth)), (depth, pos)
    seen = set()
    for c in R.gradin_cases():
        assert len(c["outs"]) == 24
        seen |= {(O["mask"], O["acc"], O["kind"]) for O in c["outs"]}
    assert seen == {(m, a, k) for m in (None, "f", "h") for a in (0, 1) for k in R.KINDS if not (a and k == "h")}
    for c in R.many_cases():
        assert {O["M"] for O in c["outs"]} == {0, 1, 65, 200} and len({O["sid"] for O in c["outs"]}) == 24
        assert sum(O["kind"] == "h" for O in c["outs"]) == 12
    assert {(c["p"], c["step"] is None) for c in R.many_cases()} == {(0.5, True), (0.5, False), (0.2, True), (0.2, False)}


def test_reference_matches_torch_float64():
    t = lambda a: torch.from_numpy(R.f64(a))
    c = R.case("torch_f", 0, [R.out(33, 9, bias=True, act=4), R.out(33, 5, act=5)], [(100, 0), (40, 1), (8, 1)])
    D = R.make_data(c)
    W = R.ref(c, D)
    y = torch.nn.functional.linear(t(D["a"][0]), t(D["b"][0]), t(D["bias"][0]))
    y[:, :4] = torch.relu(y[:, :4])
    np.testing.assert_allclose(W["y0"][0], y.numpy(), rtol=1e-12, atol=1e-13)
    y = torch.relu(torch.nn.functional.linear(torch.cat([t(D["a"][1]), t(D["a"][2])], 1), torch.cat([t(D["b"][1]), t(D["b"][2])], 1)))
    np.testing.assert_allclose(W["y1"][0], y.numpy(), rtol=1e-12, atol=1e-13)
    # grad-input through autograd: x -> relu(x) -> two linears; dZ_s are the upstream gradients, B_s = W_s^T
    c = R.case("torch_x", 1, [R.out(21, 7, act=5, mask="f", acc=1)], [(9, 0), (4, 0)], mask_scale=1.0)
    D = R.make_data(c)
    x = t(D["mask"][0]).clone().requires_grad_(True)
    h = torch.cat([torch.relu(x[:, :5]), x[:, 5:]], 1)
    loss = sum((torch.nn.functional.linear(h, t(D["b"][s]).t()) * t(D["a"][s])).sum() for s in range(2))
    loss.backward()
    np.testing.assert_allclose(R.ref(c, D)["y0"][0], (x.grad + t(D["y0"][0])).numpy(), rtol=1e-12, atol=1e-13)
    c2 = dict(c, mask_scale=1.25)
    on = R.f64(D["mask"][0])[:, :5] > 0
    want = (x.grad).numpy().copy()
    want[:, :5] = np.where(on, want[:, :5] * 1.25, 0.0)
    np.testing.assert_allclose(R.ref(c2, D)["y0"][0], want + R.f64(D["y0"][0]), rtol=1e-12, atol=1e-13)
    assert (on == 0).any() and on.any()


def test_operands_are_bf16_and_the_mask_holds_the_special_values():
    c = R.gradin_cases()[4]
    D = R.make_data(c)
    for v in list(D["a"].values()) + list(D["b"].values()) + D["mask"]:
        assert np.array_equal(R.bf16_round(v), v)
    bits = set(R.bf16_bits(D["mask"][1]).ravel().tolist())
    assert bits >= set(R.MASK_SPECIALS.tolist()), "+0, -0, the smallest positive bf16 and negative values"


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bounds_accept_the_rounded_reference_and_keep_the_figures(c):
    D = R.make_data(c)
    W = R.ref(c, D)
    assert W, "nothing to compare"
    R.check(c, R.ref(c, D, as_kernel=True), W, c["name"])
    for k, (want, bound) in W.items():
        assert (bound >= 0).all()
        if k.startswith("bn"):
            continue
        rtol, atol = Y_FIG if c["mode"] == 0 else G_FIG
        fig = atol + rtol * np.abs(want)
        if k.startswith("yh"):                                    # yh alone: the figure of y plus half a bf16 ulp, no more
            fig = fig + R.bf16_half_ulp(np.abs(want) + fig)
        assert (bound <= fig).all(), f"{c['name']} {k}: looser than the present figure"
        live = np.abs(want) > 0
        assert (bound[live] > 0).all(), f"{c['name']} {k}: a zero bound on a nonzero value"


def test_partial_sum_bounds_are_the_rows_bounds_summed():
    c = R.bn_case()
    D = R.make_data(c)
    W = R.ref(c, D)
    for o, O in enumerate(c["outs"]):
        y, b = W[f"y{o}"]
        assert W[f"bn1_{o}"][0].shape == (5, O["N"])
        for k in range(5):
            rows = slice(64 * k, min(64 * k + 64, 257))
            np.testing.assert_allclose(W[f"bn1_{o}"][0][k], y[rows].sum(0), rtol=1e-13, atol=1e-13)
            np.testing.assert_allclose(W[f"bn2_{o}"][0][k], (y[rows] ** 2).sum(0), rtol=1e-13, atol=1e-13)
            assert (W[f"bn1_{o}"][1][k] <= b[rows].sum(0) * (1 + 1e-6) + 1e-12).all()
            assert (W[f"bn2_{o}"][1][k] <= ((2 * np.abs(y[rows]) + b[rows]) * b[rows]).sum(0) * (1 + 1e-6) + 1e-12).all()


def test_bounds_reject_seeded_defects():
    seen = {d: 0 for d in R.DEFECTS}
    for c in CASES:
        if c["expect"] is not None and c["name"] not in ("auto_10",):
            continue                                               # (the large automatic launches add nothing here)
        D = R.make_data(c)
        W = R.ref(c, D)
        good = R.ref(c, D, as_kernel=True)
        assert _passes(c, good, W)
        for d in R.DEFECTS:
            B = R.ref(c, D, defect=d, as_kernel=True)
            if _same(B, good):
                continue                                           # the defect changes nothing at this launch
            assert not _passes(c, B, W), f"{c['name']}: {d} passes the bounds"
            seen[d] += 1
    assert all(seen.values()), f"defects never applied: {[d for d, n in seen.items() if not n]}"
    print("defects seen:", seen)


def test_a_defect_applies_wherever_its_path_is_taken():
    """the filter above (`changes nothing`) must not hide a defect: each one has to change the result at the launches built for it"""
    must = {"k_tail": R.geometry_cases()[:2] + R.gradin_cases()[:2], "seg_omitted": R.segment_cases(), "slab_twice": [R.ring_case()] + R.segment_cases(),
            "slab_skipped": [R.ring_case()] + R.segment_cases(), "stale_slab": [R.ring_case(), R.segment_cases()[2]],
            "next_seg_first_slab_lost": R.segment_cases()[1:], "no_bias": R.geometry_cases()[::2], "relu_extra_col": R.geometry_cases(),
            "mask_extra_col": R.gradin_cases(), "no_mask_scale": R.gradin_cases(), "acc_off": R.gradin_cases(),
            "drop_halves_swapped": R.many_cases(), "drop_tile_local_row": R.many_cases(), "stream_id_ignored": R.many_cases(),
            "step_ignored": [c for c in R.many_cases() if c["step"] is not None], "yh_truncated": R.geometry_cases() + R.gradin_cases(),
            "bn_last_row_dropped": [R.bn_case()], "bn_bias_omitted": [R.bn_case()]}
    assert set(must) == set(R.DEFECTS)
    for d, cases in must.items():
        for c in cases:
            D = R.make_data(c)
            assert not _same(R.ref(c, D, defect=d, as_kernel=True), R.ref(c, D, as_kernel=True)), f"{d} changes nothing at {c['name']}"


def test_dropout_stream_keeps_one_minus_p():
    for p in (0.5, 0.2):
        kept, total = 0, 0
        for c in R.dropout_cases():
            if c["p"] != p:
                continue
            for o, O in enumerate(c["outs"]):
                k = R.keep(c, o)[:, :min(O["act"], O["N"])]
                kept, total = kept + int(k.sum()), total + k.size
        assert total >= 10000, "too few elements to test the rate"
        sigma = np.sqrt(total * p * (1 - p))                     # (the 16-bit threshold round(p 65536) moves the mean by < 1e-5 total)
        assert abs(kept - total * (1 - p)) <= 4 * sigma, f"p = {p}: kept {kept} of {total}"
    c = R.many_cases()[0]
    a = R.keep(c, 2)
    assert (a != R.keep(dict(c, step=78), 2)).any() and (a != R.keep(dict(c, step=None), 2)).any()
    other = dict(c, outs=[dict(O, sid=O["sid"] + 1) for O in c["outs"]])
    assert (a != R.keep(other, 2)).any()
    # row r of the mask does not depend on the rows around it, column pairs share one hash
    O = c["outs"][2]
    full = R.keep_mask_bits16(R.SEED, c["step"], O["sid"] - 64, np.arange(200), O["N"], c["p"])
    assert np.array_equal(full[130:131], R.keep_mask_bits16(R.SEED, c["step"], O["sid"] - 64, np.arange(130, 131), O["N"], c["p"]))
    assert np.array_equal(a, full[:O["M"]])


def test_the_tile_choice_restated_puts_the_automatic_launches_in_every_branch():
    assert [R.auto_class(c) for c in R.auto_cases()] == [1, 7, 9, 10] == [c["expect"] for c in R.auto_cases()]
    # the direct cases themselves never reach 128-row tiles by themselves: what forcing the class is for
    assert {R.auto_class(c) for c in CASES if c["expect"] is None} <= {9, 10}


@pytest.mark.parametrize("lay", ["a", "m"])
def test_argument_blocks_are_well_formed(lay):
    from cdcmdr_amd import _lib as L
    for c in CASES:
        addr = lambda kind, i: 0x10000 + 0x1000 * (hash((kind, i)) % 4096)
        a = R.fill_args(L.G2Args(), c, lay, addr, tile_cfg=3)
        assert 0 < a.n_out == len(c["outs"]) <= L.G2_MAX_OUT and 0 < a.n_seg == len(c["segs"]) <= L.G2_MAX_SEG and a.tile_cfg == 3
        assert a.mode in (0, 1) and 0 <= a.drop_p < 1
        for s in range(a.n_seg):
            S = a.s[s]
            assert S.Kr > 0 and S.Kr % 64 == 0 and 0 <= S.out < a.n_out and S.lda >= S.Kr and S.ldb >= S.Kr
            assert S.a % 16 == 0 and S.b % 16 == 0 and S.lda % 8 == 0 and S.ldb % 8 == 0
        for o in range(a.n_out):
            O, want = a.o[o], c["outs"][o]
            assert (O.y is not None or O.yh is not None) and O.N > 0 and O.M >= 0 and not (O.accumulate and O.y is None)
            assert (O.y is None or O.ldy >= O.N + (lay == "m")) and (O.yh is None or O.ldyh >= O.N + (lay == "m"))
            assert any(S[1] == o for S in c["segs"]), "an output without a segment"
            aligned = lambda p, ld, unit: p is None or (p % 16 == 0 and ld % unit == 0)
            vec = aligned(O.y, O.ldy, 4) and aligned(O.yh, O.ldyh, 8) and aligned(O.mask, O.ldmask, 8 if O.mask_bf16 else 4)
            assert vec == (lay == "a"), "layout a takes the eight-column path, layout m the element-wise one"
            if lay == "m":                                          # not one of the pointers is on the 16-byte grid
                assert all(p is None or p % 16 for p in (O.y, O.yh, O.mask))
            assert (O.bn_partial is not None) == (want["bn"] is not None)
            if O.bn_partial is not None:
                assert a.mode == 0 and O.act_cols == 0 and O.bn_col0 >= 0 and O.bn_col0 + O.N <= O.bn_total_c
