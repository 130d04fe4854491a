"""tests/rank_ci_exact.py held to tests/rank_exact.py and tests/bootstrap_exact.py, the hand example of INTEGRATION.md, and the checks of
`eval_rank_ci` / `Evaluator(rank_ci=...)` that need no device."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import bootstrap_exact
from rank_ci_exact import rank_ci_exact
from rank_exact import FIGURES, rank_exact

KS = (1, 3, 5)


def _table(k_max):
    table = [0.0]
    for r in range(k_max):
        table.append(table[-1] + 1.0 / math.log2(r + 2))
    return np.array(table, dtype=np.float64)


def _rows(seed=11, n=900, n_user=120, n_domain=3):
    rng = np.random.default_rng(seed)
    s = np.round(rng.random(n), 1).astype(np.float32)            # eleven scores: long tie runs
    s_b = np.where(rng.random(n) < 0.5, s, np.round(rng.random(n), 1)).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.int16)
    u = rng.integers(0, n_user, size=n).astype(np.int32)
    dom = rng.integers(0, n_domain, size=n).astype(np.int32)
    w = rng.integers(1, 40, size=n_user) / 8.0                   # few mantissa bits: an integer multiple of it is exact in float64
    return y, s, s_b, u, dom, w, n_domain


def _same(a, b):
    return all(a[f][q] == b[fig][q] for f, fig in enumerate(FIGURES) for q in range(len(b[fig])))


@pytest.mark.parametrize("weighted", [False, True])
def test_point_figures_are_rank_exacts(weighted):
    y, s, s_b, u, dom, w, n_domain = _rows()
    ww = w if weighted else None
    got = rank_ci_exact(y, s, u, dom, n_domain, KS, _table(5), ww, s_b=s_b)
    for sc, key in ((s, "M"), (s_b, "M_b")):
        vals, counted, left, _ = rank_exact(y, sc, u, dom, n_domain, KS, _table(5), ww)
        for seg, g in enumerate(got):
            assert g["G"] == counted[seg] and g["left_out"] == left[seg]
            assert g["G"] >= 2 and _same(g[key], vals[seg])
    assert all(g["delta"][f][q] == g["M"][f][q] - g["M_b"][f][q] for g in got for f in range(5) for q in range(len(KS)))


@pytest.mark.parametrize("weighted", [False, True])
def test_replicates_are_rank_exact_under_the_replicate_weights(weighted):
    y, s, s_b, u, dom, w, n_domain = _rows(n=300, n_user=200)
    y[dom == 1] = 0
    y[np.flatnonzero(dom == 1)[:1]] = 1                          # domain 1: one counted user — some replicate gives it weight 0
    n_rep, seed = 12, 5
    omega = w if weighted else np.ones(len(w))
    got = rank_ci_exact(y, s, u, dom, n_domain, KS, _table(5), w if weighted else None, s_b=s_b, n_rep=n_rep, seed=seed)
    assert got[1]["G"] == 1 and got[1]["var"] is None and got[1]["var_delta"] is None and got[1]["M"] is not None
    empty = 0
    for r in range(n_rep):
        w_r = bootstrap_exact.weights(seed, r, np.arange(len(w))).astype(np.float64) * omega
        for sc, key in ((s, "reps"), (s_b, "reps_b")):
            for seg, g in enumerate(got):
                mk = np.ones(len(y), bool) if seg == n_domain else dom == seg
                users = np.unique(u[mk & (y == 1)])
                assert g["rep_counted"][r] == int((w_r[users] > 0).sum())
                if g["rep_counted"][r] == 0:
                    assert g[key][r] is None
                    empty += 1
                    continue
                vals = rank_exact(y[mk], sc[mk], u[mk], None, 1, KS, _table(5), w_r)[0][0]
                assert _same(g[key][r], vals), (r, key, seg)
    assert empty >= 2                                             # the None branch was taken (both vectors of one cell at least)


def test_unit_weights_give_the_point_figure_in_every_replicate():
    y, s, s_b, u, dom, w, n_domain = _rows()
    got = rank_ci_exact(y, s, u, dom, n_domain, KS, _table(5), w, s_b=s_b, n_rep=3, seed=9, weight_fn=bootstrap_exact.ones)
    for g in got:
        assert g["rep_counted"] == [g["G"]] * 3
        assert all(g["reps"][r] == g["M"] and g["reps_b"][r] == g["M_b"] for r in range(3))


def test_variances_against_float64_numpy():
    y, s, s_b, u, dom, w, n_domain = _rows()
    D = _table(5)
    got = rank_ci_exact(y, s, u, dom, n_domain, KS, D, w, s_b=s_b)
    for seg, g in enumerate(got):
        mk = np.ones(len(y), bool) if seg == n_domain else dom == seg
        users = np.unique(u[mk & (y == 1)])
        m = {}
        for sc, key in ((s, "a"), (s_b, "b")):                    # a user's values: rank_exact on that user's rows alone
            m[key] = np.array([[[float(v) for v in rank_exact(y[mk & (u == c)], sc[mk & (u == c)], u[mk & (u == c)], None, 1, KS, D)[0][0][fig]]
                                for fig in FIGURES] for c in users])
        ww, G = w[users][:, None, None], len(users)

        def var_of(x):
            M = (ww * x).sum(0) / ww.sum()
            return G / (G - 1) * ((ww * (x - M)) ** 2).sum(0) / ww.sum() ** 2, G / (G - 1) * (ww ** 2 * np.abs(x - M)).sum(0) / ww.sum() ** 2

        for key, x in (("var", m["a"]), ("var_b", m["b"]), ("var_delta", m["a"] - m["b"])):
            v, ab = var_of(x)
            exact, exact_abs = np.array(g[key], dtype=np.float64), np.array(g[key + "_abs"], dtype=np.float64)
            assert np.all(np.abs(v - exact) <= 1e-12 * exact + 1e-300), (seg, key)
            assert np.all(np.abs(ab - exact_abs) <= 1e-12 * exact_abs + 1e-300), (seg, key)


HAND = dict(s=np.array([0.9, 0.5, 0.5, 0.5, 0.1, 0.3, 0.7], dtype=np.float32), y=[0, 1, 0, 1, 1, 1, 0], u=[0, 0, 0, 0, 0, 1, 1])
HAND_GROUPS = ([0.257902, 2 / 9, 1 / 3, 2 / 3, 1 / 3], [0.630930, 1.0, 1 / 2, 1.0, 1 / 2])      # ndcg, recall, precision, hit, mrr at K = 2


def test_hand_example():
    assert bootstrap_exact.weights(0, 0, np.arange(2)).tolist() == [0, 2] and bootstrap_exact.weights(0, 1, np.arange(2)).tolist() == [2, 0]
    g = rank_ci_exact(HAND["y"], HAND["s"], HAND["u"], None, 1, (2,), _table(2), n_rep=2, seed=0)[1]
    assert g["G"] == 2 and g["left_out"] == 0 and g["rep_counted"] == [1, 1]
    want_var = [0.0347875, 49 / 324, 1 / 144, 1 / 36, 1 / 144]
    for f in range(5):
        m0, m1 = HAND_GROUPS[0][f], HAND_GROUPS[1][f]
        assert abs(float(g["M"][f][0]) - (m0 + m1) / 2) < 1e-6
        assert abs(float(g["var"][f][0]) - want_var[f]) < 2e-7 and abs(float(g["var"][f][0]) - (m1 - m0) ** 2 / 4) < 2e-7
        assert abs(float(g["reps"][0][f][0]) - m1) < 1e-6 and abs(float(g["reps"][1][f][0]) - m0) < 1e-6
    assert g["var"][1][0] == Fraction(49, 324) and g["var"][2][0] == Fraction(1, 144) and g["var"][3][0] == Fraction(1, 36)
    assert abs(float(g["M"][0][0]) - 0.444416) < 1e-6


def test_evaluator_rank_ci_needs_rank_at():
    from cdcmdr_amd.evaluate import Evaluator
    with pytest.raises(ValueError, match="rank_ci needs rank_at"):
        Evaluator(None, user_idx=0, n_user=4, rank_ci=True)
    with pytest.raises(ValueError, match="rank_at needs user_idx"):
        Evaluator(None, rank_at=(1,), rank_ci=True)
    ev = Evaluator(None, user_idx=0, n_user=4, rank_at=(1, 5), rank_ci=True)
    assert ev.rank_ci and not Evaluator(None, user_idx=0, n_user=4, rank_at=(1, 5)).rank_ci


def test_eval_rank_ci_argument_checks_without_a_device():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import BOOT_MAX_REP, RANK_CI_MAX_CELLS, RankCI, RankCIPaired, eval_rank_ci
    p, y, u = torch.tensor([0.5, 0.25]), torch.tensor([1, 0], dtype=torch.int16), torch.tensor([0, 0], dtype=torch.int32)
    for kw, msg in ((dict(n_user=0), "must be positive"), (dict(n_domain=0), "must be positive"),
                    (dict(n_user=(1 << 31) + 1, n_domain=1), "exceed 2\\^32"), (dict(ks=()), "cut-offs"), (dict(ks=(5, 5)), "strictly increasing"),
                    (dict(ks=(0,)), "no integer in"), (dict(n_rep=-1), "n_rep=-1"), (dict(n_rep=BOOT_MAX_REP + 1), "n_rep="),
                    (dict(n_rep=4096, n_domain=63, ks=(1, 2, 3, 4, 5)), "cells exceed"), (dict(seed=-1), "seed="), (dict(seed=1 << 64), "seed=")):
        args = dict(n_user=1, n_domain=1, ks=(1,))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            eval_rank_ci(p, y, u, **args)
    assert 4096 * 64 * 4 <= RANK_CI_MAX_CELLS < 4096 * 64 * 5
    with pytest.raises(_lib.HipExtensionError):                   # every check above passed: there is no CPU fallback
        eval_rank_ci(p, y, u, 1)
    assert RankCI._fields == ("ndcg", "recall", "precision", "hit", "mrr", "var", "counted", "left_out", "reps", "reps_b", "rep_counted")
    assert RankCIPaired._fields == RankCI._fields[:8] + ("fig_b", "var_b", "delta", "var_delta") + RankCI._fields[8:]
    assert eval_rank_ci.__doc__ and "last_err" in eval_rank_ci.__doc__
