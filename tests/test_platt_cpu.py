"""tests/platt_exact.py against closed forms and against sklearn's LogisticRegression, and the argument checks of
cdc_eval_platt_fit / cdc_eval_platt_apply, which come before any launch and so need no device."""
import re

import numpy as np
import pytest

import platt_exact as PX


def _logit(p):
    return np.log(p) - np.log1p(-p)


def test_z_and_targets():
    Z = np.log((1 - 1e-7) / 1e-7)
    z = PX.platt_z(np.array([0.0, 1.0, 0.5, 0.25, -0.1, 1.5, np.nan], np.float32))
    assert z[0] == -Z and z[1] == Z and z[2] == 0.0 and abs(z[3] + np.log(3.0)) < 1e-15 and np.isnan(z[4:]).all()
    z = PX.platt_z(np.array([np.inf, -np.inf, 1e30, -1e30, 0.5, np.nan], np.float32), "logit", 0.25)
    assert z[:5].tolist() == [np.log(3.0), -np.log(3.0), np.log(3.0), -np.log(3.0), 0.5] and np.isnan(z[5])
    t = PX.targets([1, 0, 0, 1, 0])
    assert t.tolist() == [3 / 4, 1 / 5, 1 / 5, 3 / 4, 1 / 5]
    assert PX.targets([0, 0]).tolist() == [1 / 4, 1 / 4] and PX.targets([1]).tolist() == [2 / 3]


def test_constant_score_under_bias_is_the_logit_of_the_mean_target():
    for y, c in [([1, 0, 0, 0], 0.3), ([0, 0, 0], 0.9), ([1], 0.01), ([1, 1, 0, 1, 0, 0, 0, 1, 1], 0.5)]:
        z = PX.platt_z(np.full(len(y), c, np.float32))
        for method in ("bias", "platt"):                        # platt on a single z holds a at 1 and fits b
            a, b, H, status, free = PX.fit_rows(z, y, method)
            assert a == 1.0 and free == (1,) and status == PX.CONVERGED | (PX.SLOPE_FIXED if method == "platt" else 0)
            assert abs(b - (_logit(np.mean(PX.targets(y))) - z[0])) < 1e-12


def test_two_scores_under_platt_reproduce_the_group_means():
    y = np.array([1, 0, 0, 0, 0, 1, 1, 0, 1, 0])
    p = np.array([0.1] * 5 + [0.6] * 5, np.float32)
    z = PX.platt_z(p)
    a, b, H, status, free = PX.fit_rows(z, y, "platt")
    assert status == PX.CONVERGED and free == (0, 1)
    t = PX.targets(y)
    for k in (0, 5):
        assert abs(PX.sigmoid(a * z[k] + b) - np.mean(t[k:k + 5])) < 1e-12
    # temperature with every z == 0: the gradient is zero at the start
    a, b, H, status, free = PX.fit_rows(np.zeros(4), [1, 0, 0, 1], "temperature")
    assert (a, b, status) == (1.0, 0.0, PX.CONVERGED)


def _inputs():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 63, 64, 65, 257, 4097, 16385):
        for kind in PX.KINDS:
            yield f"{kind}/{n}", PX.ctr_like(rng, n, kind)
    yield "one class", (np.array([0.2, 0.4, 0.7], np.float32), np.zeros(3, np.int16))
    yield "separable", (np.array([0.1, 0.2, 0.8, 0.9], np.float32), np.array([0, 0, 1, 1], np.int16))
    yield "ends", (np.array([0.0, 1.0, 0.0, 1.0, 0.5], np.float32), np.array([0, 1, 1, 1, 0], np.int16))


def test_the_reference_converges_inside_the_cap_and_repairs_what_was_broken():
    for what, (p, y) in _inputs():
        z = PX.platt_z(p)
        for method in PX.METHODS:
            a, b, H, status, free = PX.fit_rows(z, y, method)
            assert status & PX.CONVERGED and PX.mean_gradient(z, y, a, b, free) <= PX.REF_GTOL, (what, method)
            if "/" in what and len(y) > 1:
                assert PX.bce(z, y, a, b) <= PX.bce(z, y, 1.0, 0.0) + 2.0 / len(y), (what, method)      # the smoothing costs O(1 / m)
    assert PX.STATS["steps"] <= PX.MAX_STEPS
    rng = np.random.default_rng(1)
    p, y = PX.ctr_like(rng, 200000, "odds x10")
    a, b, _, _, _ = PX.fit_rows(PX.platt_z(p), y, "bias")
    assert abs(b + np.log(10.0)) < 0.05
    p, y = PX.ctr_like(rng, 200000, "slope 0.4 shift -1")
    a, b, _, _, _ = PX.fit_rows(PX.platt_z(p), y, "platt")
    assert abs(a - 0.4) < 0.02 and abs(b + 1.0) < 0.05


def test_apply():
    p = np.array([0.0, 0.25, 0.5, 1.0, np.nan, 1.5], np.float32)
    out = PX.platt_apply(p, 1.0, 0.0)
    assert out[:4].tolist() == [np.float32(1e-7), 0.25, 0.5, np.float32(1 - 1e-7)] and np.isnan(out[4:]).all()
    out = PX.platt_apply(p, 1.0, -np.log(3.0), eps=0.125)
    assert abs(out[2] - 0.25) < 1e-7 and out[0] == 0.125 and out[3] == 0.875 and np.isnan(out[4:]).all()


def test_against_sklearn():
    lm = pytest.importorskip("sklearn.linear_model")
    rng = np.random.default_rng(3)
    for n, kind in [(300, "calibrated"), (2000, "odds x10"), (2000, "slope 0.4 shift -1")]:
        p, y = PX.ctr_like(rng, n, kind)
        z, t = PX.platt_z(p), PX.targets(y)
        X = np.r_[z, z][:, None]
        for method in ("platt", "temperature"):
            a, b, _, _, _ = PX.fit_rows(z, y, method)
            lr = lm.LogisticRegression(penalty=None, fit_intercept=method == "platt", tol=1e-10, max_iter=10000)
            lr.fit(X, np.r_[np.ones(n), np.zeros(n)], sample_weight=np.r_[t, 1 - t])
            # 1e-5: the stopping tolerance of lbfgs, not of the code under test
            assert abs(lr.coef_[0, 0] - a) <= 1e-5 and abs(float(np.ravel(lr.intercept_)[0]) - b) <= 1e-5, (n, kind, method)


FAKE = 0x10000              # a non-null, 256-byte aligned address: every call below is refused before anything could touch it


def _fit_args(**kw):
    a = dict(score=FAKE, label=FAKE, domain=None, ld=0, n=100, n_domain=1, method=0, input=0, clip=1e-7, gtol=1e-10, max_iter=32, a=FAKE,
             b=FAKE, lb=FAKE, la=FAKE, grad=FAKE, rows=FAKE, pos=FAKE, iters=FAKE, status=FAKE, err=None, ws=FAKE, ws_bytes=0, stream=None)
    a.update(kw)
    return tuple(a.values())


def _apply_args(**kw):
    a = dict(score=FAKE, domain=None, ld=0, n=100, n_domain=1, seg=FAKE, a=FAKE, b=FAKE, input=0, clip=1e-7, eps=0.0, out=FAKE, err=None,
             stream=None)
    a.update(kw)
    return tuple(a.values())


def test_bad_arguments_are_refused_before_any_launch():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    src = open(_lib._build.INCLUDE + "/cdcmdr.h").read()
    BADARG = int(re.search(r"#define\s+CDC_E_BADARG\s+\(?(-?\d+)", src).group(1))
    TOOBIG = int(re.search(r"#define\s+CDC_E_TOOBIG\s+\(?(-?\d+)", src).group(1))
    assert BADARG < 0 and TOOBIG < 0

    def refused(fn, args, code, text):
        rc = fn(*args)
        msg = lib.cdc_last_error().decode()
        assert rc == code and text in msg, (rc, msg, text)

    fit, app = lib.cdc_eval_platt_fit, lib.cdc_eval_platt_apply
    for k in ("score", "label", "a", "b", "lb", "la", "grad", "rows", "pos", "iters", "status", "ws"):
        refused(fit, _fit_args(**{k: None}), BADARG, "eval_platt_fit: null pointer")
    for kw, text in [(dict(n=0), "bad sizes"), (dict(n=-5), "bad sizes"), (dict(n_domain=0), "bad sizes"), (dict(n_domain=1 << 20, domain=FAKE), "bad sizes"),
                     (dict(n_domain=3), "needs the domain column"), (dict(method=3), "unknown method"), (dict(method=-1), "unknown method"),
                     (dict(input=2), "unknown input"), (dict(clip=1e-13), "clip="), (dict(clip=0.3), "clip="), (dict(clip=float("nan")), "clip="),
                     (dict(gtol=0.0), "gtol="), (dict(gtol=float("nan")), "gtol="), (dict(max_iter=0), "max_iter="), (dict(max_iter=1025), "max_iter="),
                     (dict(ws=FAKE + 8), "256-byte aligned"), (dict(ws_bytes=1024), "workspace 1024 <")]:
        refused(fit, _fit_args(**kw), BADARG, text)
    refused(fit, _fit_args(n=1 << 31), TOOBIG, "exceeds 2^31")
    for k in ("score", "seg", "a", "b", "out"):
        refused(app, _apply_args(**{k: None}), BADARG, "eval_platt_apply: null pointer")
    for kw, text in [(dict(n=0), "bad sizes"), (dict(n_domain=0), "bad sizes"), (dict(n_domain=2), "needs the domain column"), (dict(input=-1), "unknown input"),
                     (dict(clip=0.5), "clip="), (dict(eps=-0.1), "eps="), (dict(eps=0.6), "eps="), (dict(eps=float("nan")), "eps=")]:
        refused(app, _apply_args(**kw), BADARG, text)
    refused(app, _apply_args(n=1 << 31), TOOBIG, "exceeds 2^31")
    assert lib.cdc_eval_platt_fit_workspace_bytes(0, 1) == 0 and lib.cdc_eval_platt_fit_workspace_bytes(10, 0) == 0
    assert lib.cdc_eval_platt_fit_workspace_bytes(1 << 31, 1) == 0
