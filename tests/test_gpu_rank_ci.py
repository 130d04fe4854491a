"""cdc_eval_rank_ci / eval_rank_ci / Evaluator(rank_ci=True) on the device against the exact rationals of tests/rank_ci_exact.py.

The bounds are derived, not measured.  u = 2^-53; every group value and every figure lies in [0, 1]; K is the cut-off, G the segment's
counted groups.  From tests/test_gpu_rank.py: a group value m_g carries at most (2 K + 3) u absolute, a figure M at most
(2 K + 2 G + 8) u — and M is checked under exactly that bound here, for both vectors (it is cdc_eval_rank's figure).

  var    the device forms t = w (m - M), adds t t over the groups and multiplies by G / (G - 1) / (den den), den = sum w.
         A centred value c = m - M is at most 1 in size, so its subtraction rounds by at most u: the computed c is off by
             E <= (2 K + 3) u + (2 K + 2 G + 8) u + u = (4 K + 2 G + 12) u.
         (c + e)^2 - c^2 = 2 c e + e^2, so with exact arithmetic behind it the scaled sum is off by at most
             2 E * [G / (G - 1) sum w^2 |c| / (sum w)^2] + E^2 * [G / (G - 1) sum w^2 / (sum w)^2] <= 2 E abs + 2 E^2,
         abs being the helper's absolute-value sum (sum w^2 <= (sum w)^2, G / (G - 1) <= 2).  The arithmetic itself is relative to
         the non-negative terms and their sum: w c, its square (twice the relative error of t, and one rounding), at most G - 1
         additions on any path of the fixed tree, den carrying G - 1 additions and entering squared, one product den den, the two
         divisions of G / (G - 1) / den^2 and the final product: 2 + 1 + (G - 1) + 2 (G - 1) + 1 + 2 + 1 = 3 G + 4 <= 3 G + 8 roundings.
             |got - want| <= 2 E abs + 2 E^2 + (3 G + 8) u want.
  var_delta   the same with c = (m_a - m_b) - delta and E doubled: two group values, two figures.
  delta  M_a - M_b of two figures within (2 K + 2 G + 8) u each, one subtraction of a value in [-1, 1]: (4 K + 4 G + 17) u.
  replicate   M_r = sum (wt w) m / sum (wt w): the figure's count with one more product per term in numerator and denominator,
         (2 K + 2 G + 10) u absolute, G the segment's counted groups (those with weight 0 add exact zeros).

Counts must be equal, NaN must stand exactly where the helper has None, and identical vectors must give delta = var_delta = 0."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from rank_ci_exact import rank_ci_exact
from rank_exact import FIGURES
from test_gpu_rank import KS_BIG, _big, _table

pytestmark = pytest.mark.gpu
U = Fraction(1, 2 ** 53)
HAND = dict(s=np.array([0.9, 0.5, 0.5, 0.5, 0.1, 0.3, 0.7], dtype=np.float32), y=[0, 1, 0, 1, 1, 1, 0], u=[0, 0, 0, 0, 0, 1, 1])


def _bf16(s):
    return torch.from_numpy(np.asarray(s, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _device(cuda, y, s, u, n_user, dom=None, n_domain=1, ks=(10,), w=None, s_b=None, n_rep=0, seed=0, strided=False):
    """-> dict of numpy arrays: out [n_stat, 5, n_k, seg], reps [n_vec, n_rep, 5, n_k, seg] or None, counted, left_out, rep_counted, err"""
    from cdcmdr_amd.evaluate import eval_rank_ci
    n = len(y)
    pred = torch.from_numpy(np.asarray(s, dtype=np.float32)).to(cuda)
    pred_b = None if s_b is None else torch.from_numpy(np.asarray(s_b, dtype=np.float32)).to(cuda)
    label = torch.from_numpy(np.asarray(y).astype(np.int16)).to(cuda)
    if strided:                                                 # user and domain as columns of one [n, 4] id matrix
        X = np.full((n, 4), -7, dtype=np.int32)
        X[:, 3] = u
        X[:, 1] = dom if dom is not None else 0
        Xd = torch.from_numpy(X).to(cuda)
        ut, dt = Xd[:, 3], (Xd[:, 1] if dom is not None else None)
        assert ut.stride(0) == 4
    else:
        ut = torch.from_numpy(np.asarray(u).astype(np.int32)).to(cuda)
        dt = None if dom is None else torch.from_numpy(np.asarray(dom).astype(np.int32)).to(cuda)
    wt = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).to(cuda)
    r = eval_rank_ci(pred, label, ut, n_user, dt, n_domain, ks, wt, pred_b=pred_b, n_rep=n_rep, seed=seed)
    return _host(r, eval_rank_ci.last_err, len(ks), n_domain, s_b is not None, n_rep)


def _host(r, err, n_k, n_domain, paired, n_rep):
    shape = (5, n_k, n_domain + 1)
    stats = [torch.stack(r[:5]), r.var] + ([r.fig_b, r.var_b, r.delta, r.var_delta] if paired else [])
    for t in stats:
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape
    assert type(r).__name__ == ("RankCIPaired" if paired else "RankCI")
    reps = None
    if n_rep:
        assert tuple(r.reps.shape) == (n_rep,) + shape and tuple(r.rep_counted.shape) == (n_rep, n_domain + 1)
        assert (r.reps_b is not None) == paired and r.rep_counted.dtype == torch.int64
        reps = torch.stack([r.reps] + ([r.reps_b] if paired else [])).cpu().numpy()
    else:
        assert r.reps is None and r.reps_b is None and r.rep_counted is None
    return dict(out=torch.stack(stats).cpu().numpy(), reps=reps, counted=r.counted.cpu().numpy(), left_out=r.left_out.cpu().numpy(),
                rep_counted=None if not n_rep else r.rep_counted.cpu().numpy(), err=int(err.item()))


def _check(got, want, ks, paired, n_rep, what=""):
    """every output against the helper (a paired reference also serves an unpaired call: the first vector's outputs are the same)"""
    assert got["err"] == 0, what
    assert got["counted"].tolist() == [g["G"] for g in want] and got["left_out"].tolist() == [g["left_out"] for g in want], what
    names = ["M", "var"] + (["M_b", "var_b", "delta", "var_delta"] if paired else [])
    assert got["out"].shape[0] == len(names)
    worst = dict.fromkeys(names + ["reps"], 0.0)
    for seg, g in enumerate(want):
        G = g["G"]
        for si, name in enumerate(names):
            a = got["out"][si, :, :, seg]
            if g[name] is None:
                assert np.isnan(a).all(), (what, seg, name, a)
                continue
            assert not np.isnan(a).any(), (what, seg, name, a)
            for f in range(5):
                for q, K in enumerate(ks):
                    exact, diff = g[name][f][q], abs(Fraction(float(a[f, q])) - g[name][f][q])
                    if name in ("M", "M_b"):
                        bound = (2 * K + 2 * G + 8) * U
                    elif name == "delta":
                        bound = (4 * K + 4 * G + 17) * U
                    else:
                        E = (4 * K + 2 * G + 12) * U * (2 if name == "var_delta" else 1)
                        bound = 2 * E * g[name + "_abs"][f][q] + 2 * E * E + (3 * G + 8) * U * exact
                    if bound:
                        worst[name] = max(worst[name], float(diff / bound))
                    assert diff <= bound, (what, seg, name, FIGURES[f], K, a[f, q], float(exact), float(diff), float(bound), G)
        if not n_rep:
            continue
        assert got["rep_counted"][:, seg].tolist() == g["rep_counted"], (what, seg)
        for vi, name in enumerate(["reps", "reps_b"][:got["reps"].shape[0]]):
            for r in range(n_rep):
                a = got["reps"][vi, r, :, :, seg]
                if g[name][r] is None:
                    assert np.isnan(a).all(), (what, seg, name, r)
                    continue
                assert not np.isnan(a).any(), (what, seg, name, r)
                for f in range(5):
                    for q, K in enumerate(ks):
                        diff, bound = abs(Fraction(float(a[f, q])) - g[name][r][f][q]), (2 * K + 2 * G + 10) * U
                        worst["reps"] = max(worst["reps"], float(diff / bound))
                        assert diff <= bound, (what, seg, name, r, FIGURES[f], K, a[f, q], float(diff), float(bound), G)
    print(what, "counted", got["counted"].tolist(), "largest error / bound", worst)


def _bits(got):
    return [None if v is None else (np.asarray(v).view(np.int64) if np.asarray(v).dtype == np.float64 else np.asarray(v))
            for k, v in sorted(got.items()) if k != "err"]


def _same_bits(a, b):
    return all((x is None and z is None) or np.array_equal(x, z) for x, z in zip(_bits(a), _bits(b)))


def test_smallest_inputs_and_the_hand_example(cuda):
    one = np.array([0.3], dtype=np.float32)
    got = _device(cuda, [1], one, [0], 1, ks=(1,))                  # one positive row: every figure 1, no variance, G = 1
    assert (got["out"][0] == 1.0).all() and np.isnan(got["out"][1]).all() and got["counted"].tolist() == [1, 1] and got["err"] == 0
    _check(got, rank_ci_exact([1], one, [0], None, 1, (1,), _table(1)), (1,), False, 0, "one positive")
    got = _device(cuda, [0], one, [0], 1, ks=(1,), s_b=one, n_rep=2)  # one negative row: everything NaN
    assert np.isnan(got["out"]).all() and np.isnan(got["reps"]).all() and got["counted"].tolist() == [0, 0] and got["left_out"].tolist() == [1, 1]
    assert (got["rep_counted"] == 0).all()
    # the hand example of INTEGRATION.md, with its two replicates
    y, s, u = HAND["y"], HAND["s"], HAND["u"]
    got = _device(cuda, y, s, u, 2, ks=(2,), n_rep=2, seed=0)
    _check(got, rank_ci_exact(y, s, u, None, 1, (2,), _table(2), n_rep=2, seed=0), (2,), False, 2, "hand")
    groups = ([0.257902, 2 / 9, 1 / 3, 2 / 3, 1 / 3], [0.630930, 1.0, 1 / 2, 1.0, 1 / 2])
    for f, v in enumerate([0.0347875, 49 / 324, 1 / 144, 1 / 36, 1 / 144]):
        assert abs(got["out"][1, f, 0, 1] - v) < 2e-7
        assert abs(got["reps"][0, 0, f, 0, 1] - groups[1][f]) < 1e-6 and abs(got["reps"][0, 1, f, 0, 1] - groups[0][f]) < 1e-6
    assert got["rep_counted"].tolist() == [[1, 1], [1, 1]]
    # signed zeros tie: one positive among two rows of one score, against a vector that separates them
    z, zb = np.array([-0.0, 0.0], dtype=np.float32), np.array([0.5, 0.25], dtype=np.float32)
    got = _device(cuda, [1, 0], z, [0, 0], 5, ks=(1, 2), s_b=zb)
    _check(got, rank_ci_exact([1, 0], z, [0, 0], None, 1, (1, 2), _table(2), s_b=zb), (1, 2), True, 0, "zeros")
    assert got["out"][0, 1, 0, 1] == 0.5 and got["out"][2, 1, 0, 1] == 1.0 and got["out"][4, 1, 0, 1] == -0.5
    # two users in two domains
    two, twob = np.array([0.3, 0.7], dtype=np.float32), np.array([0.7, 0.3], dtype=np.float32)
    got = _device(cuda, [0, 1], two, [0, 1], 2, dom=[0, 1], n_domain=2, ks=(1,), s_b=twob, n_rep=2, seed=3)
    _check(got, rank_ci_exact([0, 1], two, [0, 1], [0, 1], 2, (1,), _table(1), s_b=twob, n_rep=2, seed=3), (1,), True, 2, "two users")
    assert got["counted"].tolist() == [0, 1, 1] and got["left_out"].tolist() == [1, 0, 1]


@functools.lru_cache(maxsize=None)
def _big_want(weighted):
    n_user, n_domain, y, s, u, dom, w, _ = _big()
    return rank_ci_exact(y, s, u, dom, n_domain, KS_BIG, _table(KS_BIG[-1]), w if weighted else None, s_b=_bf16(s), n_rep=3, seed=70)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_many_small_groups_more_than_one_chunk_per_slice(cuda, weighted, paired):
    n_user, n_domain, y, s, u, dom, w, _ = _big()
    want = _big_want(weighted)
    assert want[5]["G"] == 0 and want[5]["left_out"] == 0 and want[5]["M"] is None          # the empty domain
    assert want[2]["G"] == 0 and want[2]["left_out"] > 0 and want[2]["var"] is None         # the domain without a positive
    for seg, g in enumerate(want):
        if seg not in (2, 5):
            assert g["G"] >= 2 and g["notes"]["straddle"] >= 1 and g["notes"]["straddle_b"] >= 1, seg
    assert int((dom == 4).sum()) > 64 * 256                      # domain 4's 64 slices hold more than one 256-position chunk each
    got = _device(cuda, y, s, u, n_user, dom, n_domain, KS_BIG, w if weighted else None, _bf16(s) if paired else None, n_rep=3, seed=70)
    _check(got, want, KS_BIG, paired, 3, f"70k/{weighted}/{paired}")


@functools.lru_cache(maxsize=None)
def _mid():
    n, n_user, n_domain, ks, n_rep, seed = 3000, 400, 3, (1, 4, 10), 67, 12
    rng = np.random.default_rng(3000)
    s = np.round(rng.random(n), 2).astype(np.float32)
    s_b = np.where(rng.random(n) < 0.6, s, np.round(rng.random(n), 2)).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.int16)
    u = rng.integers(0, n_user, size=n).astype(np.int32)
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    w = 0.25 + rng.random(n_user)
    want = rank_ci_exact(y, s, u, dom, n_domain, ks, _table(10), w, s_b=s_b, n_rep=n_rep, seed=seed)
    return n_user, n_domain, ks, n_rep, seed, y, s, s_b, u, dom, w, want


def test_sixty_seven_replicates_paired(cuda):
    n_user, n_domain, ks, n_rep, seed, y, s, s_b, u, dom, w, want = _mid()
    assert n_rep % 64 and n_rep > 64                             # more than one replicate tile, the last one ragged
    nan_cells = sum(g["reps"][r] is None for g in want for r in range(n_rep))
    assert nan_cells <= 1                                        # NaN cells cannot hide a failure
    got = _device(cuda, y, s, u, n_user, dom, n_domain, ks, w, s_b, n_rep, seed)
    assert int(np.isnan(got["reps"][0, :, 0, 0, :]).sum()) == nan_cells
    _check(got, want, ks, True, n_rep, "3k/67")


def test_point_figures_are_eval_ranks_and_no_output_depends_on_the_row_order(cuda):
    from cdcmdr_amd.evaluate import eval_rank
    n_user, n_domain, y, s, u, dom, w, _ = _big()
    s_b = _bf16(s)
    a = _device(cuda, y, s, u, n_user, dom, n_domain, KS_BIG, w, s_b, n_rep=3, seed=70)
    for vec, sc in ((0, s), (2, s_b)):
        r = eval_rank(torch.from_numpy(sc).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(u).to(cuda), n_user,
                      torch.from_numpy(dom).to(cuda), n_domain, KS_BIG, torch.from_numpy(w).to(cuda))
        assert np.array_equal(torch.stack(r[:5]).cpu().numpy().view(np.int64), a["out"][vec].view(np.int64))      # bit for bit, NaN included
        assert r.counted.cpu().tolist() == a["counted"].tolist() and r.left_out.cpu().tolist() == a["left_out"].tolist()
    perm = np.random.default_rng(1).permutation(len(y))
    b = _device(cuda, y[perm], s[perm], u[perm], n_user, dom[perm], n_domain, KS_BIG, w, s_b[perm], n_rep=3, seed=70)
    assert _same_bits(a, b)
    assert _same_bits(a, _device(cuda, y, s, u, n_user, dom, n_domain, KS_BIG, w, s_b, n_rep=3, seed=70))          # two calls
    assert int(np.isnan(a["out"]).sum()) == 2 * 6 * 5 * len(KS_BIG)


def test_identical_vectors_give_zero_delta_and_zero_variance(cuda):
    n_user, n_domain, ks, n_rep, seed, y, s, s_b, u, dom, w, want = _mid()
    got = _device(cuda, y, s, u, n_user, dom, n_domain, ks, w, s, n_rep=5, seed=seed)
    assert (got["out"][4] == 0.0).all() and (got["out"][5] == 0.0).all()
    assert np.array_equal(got["out"][0].view(np.int64), got["out"][2].view(np.int64))
    assert np.array_equal(got["out"][1].view(np.int64), got["out"][3].view(np.int64))
    assert np.array_equal(got["reps"][0].view(np.int64), got["reps"][1].view(np.int64))


def test_strided_id_columns_give_the_bits_of_contiguous_ones(cuda):
    n_user, n_domain, ks, n_rep, seed, y, s, s_b, u, dom, w, want = _mid()
    a = _device(cuda, y, s, u, n_user, dom, n_domain, ks, w, s_b, n_rep=5, seed=seed)
    b = _device(cuda, y, s, u, n_user, dom, n_domain, ks, w, s_b, n_rep=5, seed=seed, strided=True)
    assert _same_bits(a, b)


def test_bad_rows_set_the_error_word(cuda):
    s = np.array([0.2, 0.3, 0.7, 0.6, 0.1], dtype=np.float32)
    y, u = [0, 1, 1, 0, 1], [0, 0, 1, 1, 2]
    assert _device(cuda, y, s, u, 3, s_b=s)["err"] == 0
    bad = s.copy()
    bad[1] = np.nan
    assert _device(cuda, y, bad, u, 3)["err"] == 2
    assert _device(cuda, y, s, u, 3, s_b=bad)["err"] == 2                           # the second vector is checked too
    assert _device(cuda, y, s, [0, 0, 1, 3, 2], 3)["err"] == 4                      # user == n_user
    assert _device(cuda, y, s, [0, 0, -1, 1, 2], 3, n_rep=2)["err"] == 3
    assert _device(cuda, [0, 1, 1, 0, 2], s, u, 3)["err"] == 5                      # label 2
    assert _device(cuda, y, s, u, 3, dom=[0, 1, 2, 0, 1], n_domain=2)["err"] == 3   # domain == n_domain


def test_raw_binding_refuses_bad_arguments_before_any_launch(cuda):
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import rank_discounts
    lib = _lib.load()
    n, n_domain, n_user, n_k, n_rep = 500, 2, 40, 2, 3
    seg = n_domain + 1
    pred = torch.rand(n, device=cuda)
    label = torch.zeros(n, dtype=torch.int16, device=cuda)
    user = torch.zeros(n, dtype=torch.int32, device=cuda)
    dom = torch.zeros(n, dtype=torch.int32, device=cuda)
    ks = torch.tensor([1, 5], dtype=torch.int32, device=cuda)
    disc = rank_discounts(5, cuda)
    out = torch.full((6 * 5 * n_k * seg,), -3.0, dtype=torch.float64, device=cuda)
    reps = torch.full((2 * n_rep * 5 * n_k * seg,), -3.0, dtype=torch.float64, device=cuda)
    counts = torch.full((2 * seg,), -3, dtype=torch.int64, device=cuda)
    rep_counts = torch.full((n_rep * seg,), -3, dtype=torch.int64, device=cuda)
    err = torch.full((1,), -3, dtype=torch.int32, device=cuda)
    need = lib.cdc_eval_rank_ci_workspace_bytes(n, n_domain, n_user, n_k, 1, n_rep)
    assert need > lib.cdc_eval_rank_ci_workspace_bytes(n, n_domain, n_user, n_k, 0, n_rep) > lib.cdc_eval_rank_ci_workspace_bytes(
        n, n_domain, n_user, n_k, 0, 0) > 0
    for bad in ((n, n_domain, n_user, 0, 0, 0), (n, n_domain, n_user, 9, 0, 0), (n, n_domain, n_user, n_k, 0, 4097), (n, n_domain, n_user, n_k, 0, -1),
                (n, n_domain, 1 << 31, n_k, 0, 0), (1 << 31, n_domain, n_user, n_k, 0, 0), (n, 63, n_user, 5, 0, 4096)):
        assert lib.cdc_eval_rank_ci_workspace_bytes(*bad) == 0, bad
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pred=pred.data_ptr(), pred_b=pred.data_ptr(), label=label.data_ptr(), user=user.data_ptr(), n_user=n_user, domain=dom.data_ptr(),
                n_domain=n_domain, ks=ks.data_ptr(), n_k=n_k, disc=disc.data_ptr(), n=n, n_rep=n_rep, out=out.data_ptr(), reps=reps.data_ptr(),
                counts=counts.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cdc_eval_rank_ci(a["pred"], a["pred_b"], a["label"], a["user"], 1, a["n_user"], a["domain"], 1, a["n_domain"], None, a["ks"],
                                    a["n_k"], a["disc"], a["n"], a["n_rep"], 7, a["out"], a["reps"], a["counts"], rep_counts.data_ptr(),
                                    err.data_ptr(), a["ws"], a["ws_bytes"], stream)

    for kw in ({"pred": None}, {"label": None}, {"user": None}, {"ks": None}, {"disc": None}, {"out": None}, {"counts": None}, {"ws": None},
               {"domain": None}, {"n": 0}, {"n_domain": 0}, {"n_user": 0}, {"n_k": 0}, {"n_k": 9}, {"n_rep": -1}, {"n_rep": 4097}, {"reps": None},
               {"n_rep": 0}, {"n_user": 1 << 31}, {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": ws.data_ptr() + 8},
               {"n_rep": 4096, "n_domain": 63, "n_k": 5}):
        assert call(**kw) == -1, kw                             # CDC_E_BADARG ({"n_rep": 0}: a replicate array without replicates)
    assert call(n=1 << 31) == -2 and b"2^31" in lib.cdc_last_error()      # CDC_E_TOOBIG
    torch.cuda.synchronize()
    assert (out == -3.0).all() and (reps == -3.0).all() and (counts == -3).all() and (rep_counts == -3).all()
    assert int(err.item()) == -3 and not ws.any()                # nothing ran
    err.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0, 1, 0, 1] and int(err.item()) == 0 and bool(torch.isnan(out).all())


def test_replays_from_a_captured_graph(cuda):
    from cdcmdr_amd.evaluate import eval_rank_ci
    n, n_user, n_domain, ks, n_rep = 3000, 200, 3, (1, 10), 5
    rng = np.random.default_rng(9)

    def draw():
        s = np.round(rng.random(n), 2).astype(np.float32)
        return (s, np.where(rng.random(n) < 0.5, s, np.float32(0.5)).astype(np.float32), rng.integers(0, 2, size=n).astype(np.int16),
                rng.integers(0, n_user, size=n).astype(np.int32), rng.integers(0, n_domain, size=n).astype(np.int32))
    first, second = draw(), draw()
    w = 0.25 + rng.random(n_user)
    bufs = [torch.from_numpy(a).to(cuda) for a in first]
    wt = torch.from_numpy(w).to(cuda)

    def run():
        return eval_rank_ci(bufs[0], bufs[2], bufs[3], n_user, bufs[4], n_domain, ks, wt, pred_b=bufs[1], n_rep=n_rep, seed=4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up outside the capture: library load, allocator, the cached tables
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = run()
        err = eval_rank_ci.last_err
    for data in (second, first):
        for t, a in zip(bufs, data):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        got = _host(r, err, len(ks), n_domain, True, n_rep)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(got, _host(r, err, len(ks), n_domain, True, n_rep))
        eager = run()
        assert _same_bits(got, _host(eager, eval_rank_ci.last_err, len(ks), n_domain, True, n_rep))
        s, s_b, y, u, dom = data
        _check(got, rank_ci_exact(y, s, u, dom, n_domain, ks, _table(10), w, s_b=s_b, n_rep=n_rep, seed=4), ks, True, n_rep, "graph")


def test_evaluator_rank_ci(cuda):
    from cdcmdr_amd.evaluate import Evaluator, eval_rank_ci, summarize_bootstrap
    from cdcmdr_amd.model.mmoe import MMoE
    FD = [30, 2000, 7, 300, 3]                                  # column 3: 300 users, column 4: 3 domains
    ks = (1, 10)
    torch.manual_seed(3)
    model = MMoE(FD, 8, 3, 4, (32, 16), (8,), dropout=0.2).to(cuda).set_precision("f32")
    rng = np.random.default_rng(5)
    n, bs = 2500, 1024
    X = np.stack([rng.integers(0, d, size=n) for d in FD], axis=1).astype(np.int32)
    y = rng.integers(0, 2, size=n).astype(np.int16)
    g = X[:, 4].astype(np.int64)
    loader = [(torch.from_numpy(X[i:i + bs]).to(cuda), torch.from_numpy(y[i:i + bs]).to(cuda).reshape(-1, 1),
               torch.from_numpy(g[i:i + bs]).to(cuda).reshape(-1, 1)) for i in range(0, n, bs)]
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    wv = torch.tensor([w[d] for d in range(3)], dtype=torch.float64, device=cuda)
    kw = dict(mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w, user_idx=3, n_user=300, rank_at=ks)
    names = [f"{f}@{K}" for f in FIGURES for K in ks]
    se_keys = [f"{p}_{k}_se" for p in ("total", "domain") for k in names]
    boot_keys = [f"{p}_{k}_boot_{x}" for p in ("total", "domain", "mean") for k in names for x in ("se", "lo", "hi")]
    # test(): analytic
    res0 = Evaluator(model, **kw).test(loader)
    ev = Evaluator(model, rank_ci=True, **kw)
    res = ev.test(loader)
    assert sorted(res) == sorted(list(res0) + se_keys)
    assert all(res[k] == res0[k] for k in res0)                 # the old keys keep their bits
    pred, label, dom, user = ev._score(loader)
    r = eval_rank_ci(pred, label, user, 300, dom, 3, ks)
    var = r.var.cpu().numpy()
    for f, fig in enumerate(FIGURES):
        for q, K in enumerate(ks):
            assert res[f"total_{fig}@{K}_se"] == np.sqrt(var[f, q, 3]) and (K > 1 or res[f"total_{fig}@{K}_se"] > 0)    # K = 10 covers most lists
            assert res[f"domain_{fig}@{K}_se"] == {d: np.sqrt(var[f, q, d]) for d in range(3)}
    # test(): with bootstrap
    res0 = Evaluator(model, bootstrap=16, bootstrap_seed=5, bootstrap_level=0.9, **kw).test(loader)
    evb = Evaluator(model, rank_ci=True, bootstrap=16, bootstrap_seed=5, bootstrap_level=0.9, **kw)
    res = evb.test(loader)
    assert sorted(res) == sorted(list(res0) + se_keys + boot_keys)
    assert all(res[k] == res0[k] for k in res0 if k != "boot_valid") and res["boot_valid"] <= res0["boot_valid"]
    reps = eval_rank_ci(pred, label, user, 300, dom, 3, ks, n_rep=16, seed=5).reps
    for f, fig in enumerate(FIGURES):
        for q, K in enumerate(ks):
            x = reps[:, f, q]
            mean = (x[:, :3] * wv).sum(1)                       # formed per replicate on the host side of the call
            se, lo, hi, _ = (t.cpu().tolist() for t in summarize_bootstrap(torch.cat([x, mean[:, None]], 1), 0.9))
            for what, v in (("se", se), ("lo", lo), ("hi", hi)):
                assert res[f"total_{fig}@{K}_boot_{what}"] == v[3] and res[f"mean_{fig}@{K}_boot_{what}"] == v[4]
                assert res[f"domain_{fig}@{K}_boot_{what}"] == {d: v[d] for d in range(3)}
            assert K > 1 or res[f"mean_{fig}@{K}_boot_se"] > 0
    # compare(): against itself, then against the bf16 pass
    base = Evaluator(model, **kw)
    cmp0 = base.compare(base, loader)
    delta_keys = [f"{p}_{k}_{x}" for p in ("total", "domain") for k in names for x in ("delta", "delta_se", "z")]
    same = ev.compare(ev, loader)
    assert sorted(same) == sorted(list(cmp0) + delta_keys)
    for k in names:
        assert same[f"total_{k}_delta"] == 0.0 and same[f"total_{k}_delta_se"] == 0.0 and np.isnan(same[f"total_{k}_z"])
        assert all(v == 0.0 for v in same[f"domain_{k}_delta_se"].values()) and all(np.isnan(v) for v in same[f"domain_{k}_z"].values())
    other = Evaluator(model, precision="bf16", **kw)
    cmp0 = Evaluator(model, bootstrap=16, bootstrap_seed=5, bootstrap_level=0.9, **kw).compare(other, loader)
    both = evb.compare(other, loader)
    more = [f"{p}_{k}_delta_boot_{x}" for p in ("total", "domain", "mean") for k in names for x in ("se", "lo", "hi")]
    more += [f"mean_{k}_{x}" for k in names for x in ("delta", "z")]
    assert sorted(both) == sorted(list(cmp0) + delta_keys + more)
    assert all(both[k] == cmp0[k] for k in cmp0 if k != "boot_valid")          # the old keys keep their bits (bf16 against f32: no NaN)
    pb = other.predict(loader)[0]
    pair = eval_rank_ci(pred, label, user, 300, dom, 3, ks, pred_b=pb, n_rep=16, seed=5)
    d_reps, delta, var_d = pair.reps - pair.reps_b, pair.delta.cpu().numpy(), pair.var_delta.cpu().numpy()
    for f, fig in enumerate(FIGURES):
        for q, K in enumerate(ks):
            k = f"{fig}@{K}"
            assert both[f"total_{k}_delta"] == delta[f, q, 3] and both[f"total_{k}_delta_se"] == np.sqrt(var_d[f, q, 3])
            assert both[f"domain_{k}_delta"] == {d: delta[f, q, d] for d in range(3)}
            x = d_reps[:, f, q]
            se = summarize_bootstrap(torch.cat([x, (x[:, :3] * wv).sum(1)[:, None]], 1), 0.9)[0].cpu().tolist()
            assert both[f"total_{k}_delta_boot_se"] == se[3] and both[f"mean_{k}_delta_boot_se"] == se[4]
            mean_delta = sum(w[d] * delta[f, q, d] for d in range(3))
            assert both[f"mean_{k}_delta"] == mean_delta
            if se[4] > 0:
                assert both[f"mean_{k}_z"] == mean_delta / se[4]
    with pytest.raises(ValueError, match="different user columns"):
        ev.compare(Evaluator(model, mode="multi", domain_idx=4, n_domain=3, domain_cnt_weight=w), loader)
