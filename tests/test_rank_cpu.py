"""The per-user top-K figures without a GPU: the closed forms of tests/rank_exact.py against brute-force enumeration of every order
of the tied rows and against sklearn's ndcg_score, the hand example of INTEGRATION.md, the discount table, the argument checks of
cdc_eval_rank (which come before anything touches a device), eval_rank's and Evaluator's own checks, and Runner's select_by rule."""
import ctypes as C
import decimal
import math
import os
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from rank_exact import FIGURES, brute_force, exact_table, group_figures, rank_exact, user_runs

KS = (1, 2, 3, 5, 10)


def _table(k_max):
    from cdcmdr_amd.evaluate import rank_discounts
    return rank_discounts(k_max).numpy()


def _random_groups(n_groups, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n_groups):
        rows = int(rng.integers(1, 8))
        s = rng.integers(0, 3, size=rows).astype(np.float32) / 2          # three scores: heavy ties
        y = (rng.random(rows) < 0.5).astype(np.int64)
        if y.sum() == 0:
            y[rng.integers(0, rows)] = 1
        yield y, s


def test_closed_forms_equal_brute_force_over_every_order_of_the_tied_rows():
    D = exact_table(_table(10))
    seen = 0
    for y, s in _random_groups(400, 7):
        (_, runs), = user_runs(y, s, np.zeros(len(y), dtype=np.int64))
        assert sum(t for t, _ in runs) == len(y) and sum(p for _, p in runs) == int(y.sum())
        closed, brute = group_figures(runs, KS, D), brute_force(runs, KS, D)
        for f in FIGURES:
            assert closed[f] == brute[f], (f, runs, closed[f], brute[f])
        seen += any(t > 1 and 0 < p < t for t, p in runs)
    assert seen > 100                                           # mixed tie runs are the rule, not the exception


def test_ndcg_equals_sklearn_ndcg_score():
    metrics = pytest.importorskip("sklearn.metrics")
    table = _table(10)
    D = exact_table(table)
    worst = 0.0
    for y, s in _random_groups(300, 11):
        if len(y) < 2:
            continue                                            # ndcg_score refuses a single document
        (_, runs), = user_runs(y, s, np.zeros(len(y), dtype=np.int64))
        ours = group_figures(runs, KS, D)["ndcg"]
        for q, K in enumerate(KS):
            ref = metrics.ndcg_score(y.reshape(1, -1), s.reshape(1, -1).astype(np.float64), k=K, ignore_ties=False)
            worst = max(worst, abs(float(ours[q]) - ref))
    print("largest |ndcg - sklearn|", worst)
    assert worst <= 1e-12


def _hand():
    s = np.array([0.9, 0.5, 0.5, 0.5, 0.1, 0.3, 0.7], dtype=np.float32)
    y = [0, 1, 0, 1, 1, 1, 0]
    u = [0, 0, 0, 0, 0, 1, 1]
    return y, s, u


def test_hand_example():
    y, s, u = _hand()
    table = _table(3)
    assert table[1] == 1.0 and table[2] == 1.6309297535714575
    D = exact_table(table)
    assert dict(user_runs(y, s, u)) == {0: ((1, 0), (3, 2), (1, 1)), 1: ((1, 0), (1, 1))}
    u0, u1 = group_figures(((1, 0), (3, 2), (1, 1)), (2, 3), D), group_figures(((1, 0), (1, 1)), (2, 3), D)
    assert [u0[f][0] for f in FIGURES[1:]] == [Fraction(2, 9), Fraction(1, 3), Fraction(2, 3), Fraction(1, 3)]
    assert u0["ndcg"][0] == Fraction(2, 3) * (D[2] - D[1]) / D[2] and abs(float(u0["ndcg"][0]) - 0.257902) < 5e-7
    assert [u1[f][0] for f in FIGURES[1:]] == [1, Fraction(1, 2), 1, Fraction(1, 2)]
    assert abs(float(u1["ndcg"][0]) - 0.630930) < 5e-7
    assert [u0[f][1] for f in FIGURES[1:]] == [Fraction(4, 9), Fraction(4, 9), 1, Fraction(4, 9)]       # K = 3
    assert abs(float(u0["ndcg"][1]) - 0.353814) < 5e-7
    vals, counted, left, _ = rank_exact(y, s, u, None, 1, (2,), table)
    assert counted == [2, 2] and left == [0, 0]
    for seg in vals:
        assert [seg[f][0] for f in FIGURES[1:]] == [Fraction(11, 18), Fraction(5, 12), Fraction(5, 6), Fraction(5, 12)]
        assert abs(float(seg["ndcg"][0]) - 0.444416) < 5e-7
    # a weight per user, and a user without a positive is left out
    vals, counted, left, _ = rank_exact(y + [0], np.r_[s, np.float32(0.4)], u + [2], None, 1, (2,), table, weights=[0.5, 1.5, 9.0])
    assert counted == [2, 2] and left == [1, 1]
    assert vals[1]["recall"][0] == (Fraction(1, 2) * Fraction(2, 9) + Fraction(3, 2)) / 2


def test_rank_discounts_table():
    from cdcmdr_amd.evaluate import rank_discounts
    table = rank_discounts(1024)
    assert table.dtype == torch.float64 and table.shape == (1025,) and rank_discounts(1024) is table
    want = [0.0]
    for r in range(1024):
        want.append(want[-1] + 1.0 / math.log2(r + 2))
    assert table.tolist() == want                               # the sequential float64 recurrence, bit for bit
    assert rank_discounts(10).tolist() == want[:11]
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        ln2, acc = decimal.Decimal(2).ln(), decimal.Decimal(0)
        for r in range(1024):
            acc += ln2 / decimal.Decimal(r + 2).ln()
            rel = abs(decimal.Decimal(want[r + 1]) - acc) / acc
            assert rel <= decimal.Decimal(1024) * decimal.Decimal(2) ** -52, (r, rel)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match=str(bad)):
            rank_discounts(bad)


def test_eval_rank_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, 256-byte aligned, never dereferenced on the host
    big = 1 << 40

    def call(pred=p, label=p, user=p, n_user=100, domain=p, n_domain=3, ks=p, n_k=3, disc=p, n=10, out=p, counts=p, ws=p, ws_bytes=big):
        return lib.cdc_eval_rank(pred, label, user, 1, n_user, domain, 1, n_domain, None, ks, n_k, disc, n, out, counts, None, ws,
                                 ws_bytes, None)

    for kw in ({"pred": None}, {"label": None}, {"user": None}, {"ks": None}, {"disc": None}, {"out": None}, {"counts": None},
               {"ws": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.cdc_last_error(), kw
    for n_k in (0, 9, -1):
        assert call(n_k=n_k) == -1 and b"cut-offs" in lib.cdc_last_error(), n_k
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    assert call(n_user=(1 << 30) + 1) == -1 and b"exceed 2^32" in lib.cdc_last_error()          # 4 * (2^30 + 1) > 2^32
    assert call(n_user=1 << 32, n_domain=1, domain=None) == -1 and b"exceed 2^32" in lib.cdc_last_error()
    assert call(n=1 << 31) == -1 and b"bad sizes" in lib.cdc_last_error()
    assert call(n=0) == -1 and call(n_user=0) == -1 and call(n_domain=0) == -1
    assert call(ws_bytes=1024) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    size = lib.cdc_eval_rank_workspace_bytes
    assert size(0, 3, 100, 3) == 0 and size(10, 3, (1 << 30) + 1, 3) == 0 and size(10, 3, 100, 0) == 0 and size(10, 3, 100, 9) == 0


def test_eval_rank_host_mirror_checks_arguments():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import Evaluator, eval_rank
    pred, label, user = torch.rand(4), torch.zeros(4, dtype=torch.int16), torch.zeros(4, dtype=torch.int32)
    for ks, word in (((10, 5), "strictly increasing"), ((5, 5), "strictly increasing"), ((0, 5), "0"), ((1, 1025), "1025"),
                     ((), "0 cut-offs"), (tuple(range(1, 10)), "9 cut-offs"), ((2.5,), "2.5")):
        with pytest.raises(ValueError, match=word):
            eval_rank(pred, label, user, n_user=10, ks=ks)
    with pytest.raises(ValueError, match="2\\^32"):
        eval_rank(pred, label, user, n_user=1 << 31, domain=user, n_domain=2)
    with pytest.raises(_lib.HipExtensionError):
        eval_rank(pred, label, user, n_user=10, ks=(1, 10))
    with pytest.raises(ValueError, match="user_idx"):
        Evaluator(None, rank_at=10)
    with pytest.raises(ValueError, match="1025"):
        Evaluator(None, user_idx=1, n_user=4, rank_at=(1, 1025))
    assert Evaluator(None, user_idx=1, n_user=4, rank_at=10).rank_at == (10,)
    assert Evaluator(None, user_idx=1, n_user=4, rank_at=[1, 10]).rank_at == (1, 10)
    assert Evaluator(None, user_idx=1, n_user=4).rank_at is None


def _runner(tmp_path, **kw):
    from cdcmdr_amd.runner import Runner
    step = types.SimpleNamespace(opt=types.SimpleNamespace(state_dict=lambda: {}, flush_table=lambda: None))
    return Runner(torch.nn.Linear(2, 1), step, None, os.path.join(tmp_path, "best.pth.tar"), num_trials=2, log=lambda *_: None, **kw)


def _result(mean_auc, **more):
    r = {"total_auc": 0.6, "total_loss": 0.5, "mean_auc": mean_auc, "mean_loss": 0.5}
    r.update(more)
    return r


def test_runner_selects_by_a_rank_figure(tmp_path):
    from cdcmdr_amd.runner import Runner
    key = "mean_ndcg@10"
    r = _runner(tmp_path, select_by=key)
    assert r.is_continuable(_result(0.9, **{key: 0.31}), 0) and r.trial_counter == 0 and r.best_select == 0.31
    ck = torch.load(r.save_model_path, weights_only=False)
    assert ck["epoch"] == 1 and ck["select_by"] == key and ck["best_mean_ndcg@10"] == 0.31
    assert r.is_continuable(_result(0.95, **{key: 0.30}), 1) and r.trial_counter == 1          # mean_auc rose, the figure fell: a trial
    assert torch.load(r.save_model_path, weights_only=False)["epoch"] == 1
    assert r.is_continuable(_result(0.5, **{key: 0.32}), 2) and r.trial_counter == 0 and r.best_select == 0.32
    assert torch.load(r.save_model_path, weights_only=False)["epoch"] == 3
    assert r.is_continuable(_result(0.99, **{key: 0.2}), 3) and not r.is_continuable(_result(0.99, **{key: float("nan")}), 4)   # early stop
    r = _runner(tmp_path, select_by="total_mrr@5")
    assert r.is_continuable(_result(0.9, **{"total_mrr@5": 0.4}), 0) and r.best_select == 0.4
    for ok in ("total_hit@1", "mean_recall@1024", "mean_precision@50"):
        _runner(tmp_path, select_by=ok)
    # an evaluator without rank_at cannot serve the key
    r = _runner(tmp_path, select_by=key)
    with pytest.raises(KeyError, match="rank_at"):
        r.is_continuable(_result(0.6, total_gauc=0.5), 0)
    for bad in ("total_auc", "mean_ndcg", "mean_ndcg@", "mean_ndcg@0", "mean_map@10", "domain_ndcg@10", "mean_ndcg@10 ", 10):
        with pytest.raises(ValueError):
            Runner(None, None, None, "x", select_by=bad)
