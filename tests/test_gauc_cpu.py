"""GAUC without a GPU: the exact helper (tests/gauc_exact.py) against the reference's own figures
(tests/golden/g18_gauc.npz: gauc_score of base.py:33-64 captured in the reference's environment, tools/make_golden_gauc.py),
the argument checks of cdc_eval_gauc, which come before anything touches a device, and Runner's select_by rule.

The bound of the helper against the fixture is 1e-12 relative, the project's figure for sklearn-derived goldens (g9): the
reference sums one rounded roc_auc_score per user in float, the helper is exact."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest
import torch

from gauc_exact import as_float, gauc_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g18_gauc.npz")


def test_exact_helper_equals_the_reference_on_g18():
    d = np.load(GOLD)
    n_domain = int(d["n_domain"])
    assert len(d["scores"]) == 500 and n_domain == 4 and int(d["n_user"]) == 42
    weights = {k: float(v) for k, v in enumerate(d["weights"])}
    for tag, w in (("none", None), ("w", weights)):
        vals, counted, left = gauc_exact(d["targets"], d["scores"], d["users"], d["domains"], n_domain, w)
        for k in range(n_domain + 1):
            want = float(d[f"gauc_all_{tag}" if k == n_domain else f"gauc_d{k}_{tag}"])
            got = as_float(vals[k])
            if math.isnan(want):
                assert vals[k] is None and counted[k] == 0 and left[k] > 0, (tag, k)      # the reference's division by zero
            else:
                assert abs(got - want) <= 1e-12 * abs(want), (tag, k, got, want)
                assert counted[k] > 0
    # what the fixture was built to contain
    assert math.isnan(float(d["gauc_d3_none"])) and math.isnan(float(d["gauc_d3_w"]))
    assert int((d["users"] == 40).sum()) == 1 and len(set(d["targets"][d["users"] == 41])) == 1
    z = d["scores"][d["users"] == 7]
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert not np.allclose(d["weights"], np.round(d["weights"]))


def test_exact_helper_on_hand_computed_groups():
    # user 0: scores .1(-) .5(+) .5(-) .9(+) -> U = 1.5 + 2 = 3.5 of 4; user 1: one class; user 2: -0.0(+) ties +0.0(-) -> 0.5
    y = [0, 1, 0, 1, 1, 1, 1, 0]
    s = np.array([.1, .5, .5, .9, .3, .4, -0.0, 0.0], dtype=np.float32)
    u = [0, 0, 0, 0, 1, 1, 2, 2]
    vals, counted, left = gauc_exact(y, s, u)
    assert counted == [2, 2] and left == [1, 1]
    from fractions import Fraction
    assert vals[0] == vals[1] == (4 * Fraction(7, 8) + 2 * Fraction(1, 2)) / 6
    vals, _, _ = gauc_exact(y, s, u, weights={0: 0.5, 1: 7.0, 2: 1.5})
    assert vals[1] == (Fraction(1, 2) * Fraction(7, 8) + Fraction(3, 2) * Fraction(1, 2)) / 2


def test_eval_gauc_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, 256-byte aligned, never dereferenced on the host
    big = 1 << 40

    def call(pred=p, label=p, user=p, n_user=100, domain=p, n_domain=3, n=10, out=p, counts=p, ws=p, ws_bytes=big):
        return lib.cdc_eval_gauc(pred, label, user, 1, n_user, domain, 1, n_domain, None, n, out, counts, None, ws, ws_bytes, None)

    for kw in ({"pred": None}, {"label": None}, {"user": None}, {"out": None}, {"counts": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.cdc_last_error(), kw
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    assert call(n_user=(1 << 30) + 1) == -1 and b"exceed 2^32" in lib.cdc_last_error()          # 4 * (2^30 + 1) > 2^32
    assert call(n_user=1 << 32, n_domain=1, domain=None) == -1 and b"exceed 2^32" in lib.cdc_last_error()
    assert call(n=1 << 31) == -1 and b"bad sizes" in lib.cdc_last_error()
    assert call(n=0) == -1 and call(n_user=0) == -1 and call(n_domain=0) == -1
    assert call(ws_bytes=1024) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    assert lib.cdc_eval_gauc_workspace_bytes(0, 3, 100) == 0 and lib.cdc_eval_gauc_workspace_bytes(10, 3, (1 << 30) + 1) == 0


def test_eval_gauc_host_mirror_checks_arguments():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import Evaluator, eval_gauc
    pred, label, user = torch.rand(4), torch.zeros(4, dtype=torch.int16), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="2\\^32"):
        eval_gauc(pred, label, user, n_user=1 << 31, domain=user, n_domain=2)
    with pytest.raises(_lib.HipExtensionError):
        eval_gauc(pred, label, user, n_user=10)
    with pytest.raises(ValueError, match="n_user"):
        Evaluator(None, user_idx=1)
    ev = Evaluator(None, user_idx=1, n_user=4, user_weight={0: 0.5, 2: 1.25})
    w = ev.user_weight.tolist()
    assert w[0] == 0.5 and w[2] == 1.25 and math.isnan(w[1]) and math.isnan(w[3])


def _runner(tmp_path, **kw):
    from cdcmdr_amd.runner import Runner
    step = types.SimpleNamespace(opt=types.SimpleNamespace(state_dict=lambda: {}, flush_table=lambda: None))
    return Runner(torch.nn.Linear(2, 1), step, None, os.path.join(tmp_path, "best.pth.tar"), num_trials=2, log=lambda *_: None, **kw)


def _result(mean_auc, total_gauc, mean_gauc=None):
    r = {"total_auc": 0.6, "total_loss": 0.5, "mean_auc": mean_auc, "mean_loss": 0.5, "total_gauc": total_gauc}
    if mean_gauc is not None:
        r["mean_gauc"] = mean_gauc
    return r


def test_runner_select_by(tmp_path):
    from cdcmdr_amd.runner import Runner
    # total_gauc decides, although mean_auc moves the other way
    r = _runner(tmp_path, select_by="total_gauc")
    assert r.is_continuable(_result(0.9, 0.55), 0) and r.trial_counter == 0 and r.best_select == 0.55
    ck = torch.load(r.save_model_path, weights_only=False)
    assert ck["epoch"] == 1 and ck["select_by"] == "total_gauc" and ck["best_total_gauc"] == 0.55
    assert r.is_continuable(_result(0.95, 0.54), 1) and r.trial_counter == 1           # worse GAUC: a trial, no new checkpoint
    assert torch.load(r.save_model_path, weights_only=False)["epoch"] == 1
    assert r.is_continuable(_result(0.5, 0.56), 2) and r.trial_counter == 0 and r.best_select == 0.56
    assert torch.load(r.save_model_path, weights_only=False)["epoch"] == 3
    assert r.is_continuable(_result(0.99, 0.50), 3) and not r.is_continuable(_result(0.99, float("nan")), 4)   # NaN never improves
    # mean_gauc likewise
    r = _runner(tmp_path, select_by="mean_gauc")
    assert r.is_continuable(_result(0.9, 0.5, mean_gauc=0.6), 0) and r.best_select == 0.6
    assert r.is_continuable(_result(0.95, 0.9, mean_gauc=0.59), 1) and r.trial_counter == 1
    # None keeps the reference's rule
    r = _runner(tmp_path)
    assert r.is_continuable(_result(0.7, 0.1), 0) and r.best_mean_auc == 0.7
    assert r.is_continuable(_result(0.6, 0.9), 1) and r.trial_counter == 1
    assert "select_by" not in torch.load(r.save_model_path, weights_only=False)
    # an evaluator without a user column cannot serve the key
    r = _runner(tmp_path, select_by="mean_gauc")
    with pytest.raises(KeyError, match="user_idx"):
        r.is_continuable({"total_auc": 0.6, "total_loss": 0.5, "mean_auc": 0.6, "mean_loss": 0.5}, 0)
    with pytest.raises(ValueError):
        Runner(None, None, None, "x", select_by="total_auc")
