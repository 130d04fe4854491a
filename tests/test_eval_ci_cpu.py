"""Standard errors of log-loss and GAUC without a GPU: the two exact forms of tests/gauc_ci_exact.py against each other and against
hand-worked cases, tests/loss_ci_exact.py against hand-worked cases, the argument checks of cdc_eval_loss_ci / cdc_eval_gauc_ci (they
come before anything touches a device), and the host side of eval_loss_ci / eval_gauc_ci / Evaluator."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from gauc_ci_exact import gauc_ci_brute, gauc_ci_exact, gauc_ci_rows
from gauc_exact import gauc_rows
from loss_ci_exact import loss_ci_exact, loss_ci_rows, loss_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUC_KEYS = ("gauc", "var", "gauc_b", "var_b", "delta", "var_delta")


@pytest.mark.parametrize("n,n_user,levels,seed", [(2, 1, 2, 0), (9, 3, 2, 1), (40, 5, 3, 2), (120, 8, 5, 3), (300, 40, 5, 4), (300, 7, 1000, 5)])
@pytest.mark.parametrize("weighted", [False, True])
def test_brute_force_equals_the_moment_form(n, n_user, levels, seed, weighted):
    rng = np.random.default_rng(seed)
    s = (rng.integers(0, levels, size=n) / levels).astype(np.float32)              # heavy ties
    sb = np.where(rng.random(n) < 0.3, (rng.integers(0, levels, size=n) / levels).astype(np.float32), s)
    s[: n // 3][s[: n // 3] == 0] = -0.0                                            # signed zeros tie
    y = (rng.random(n) < 0.4).astype(np.int16)
    u = rng.integers(0, n_user, size=n)
    if n_user > 2:
        y[u == 1] = 1                                                               # a single-class user
    w = (0.25 + rng.random(n_user)) if weighted else None
    a, b = gauc_ci_brute(y, s, u, w, sb), gauc_ci_rows(y, s, u, w, sb)
    for k in GAUC_KEYS + ("counted", "left_out"):
        assert a[k] == b[k], (k, a[k], b[k])
    one = gauc_ci_rows(y, s, u, w)
    assert one["gauc"] == a["gauc"] and one["var"] == a["var"] and "gauc_b" not in one
    g, counted, left = gauc_rows(y, s, u, w)                                        # and the GAUC helper that already exists
    assert (g, counted, left) == (a["gauc"], a["counted"], a["left_out"])
    dom = rng.integers(0, 3, size=n)
    for x, z in zip(gauc_ci_exact(y, s, u, dom, 3, w, sb), gauc_ci_exact(y, s, u, dom, 3, w, sb, rows=gauc_ci_brute)):
        assert all(x[k] == z[k] for k in GAUC_KEYS)


def test_the_worked_gauc_example():
    # user 0: positives {0.9, 0.4}, negatives {0.5, 0.1, 0.4}: 2U = 9 of 12, A = 3/4, 5 rows
    # user 1: positive {0.2}, negative {0.7}: A = 0, 2 rows;   user 2: one class, left out
    # user 3: positive {0.5}, negatives {0.5, 0.1}: 2U = 3 of 4, A = 3/4, 3 rows
    y = [1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0]
    s = np.array([0.9, 0.5, 0.4, 0.1, 0.4, 0.2, 0.7, 0.3, 0.5, 0.5, 0.1], dtype=np.float32)
    u = [0, 0, 0, 0, 0, 1, 1, 2, 3, 3, 3]
    G = Fraction(5 * 3, 4 * 10) + Fraction(3 * 3, 4 * 10)                           # (5 * 3/4 + 2 * 0 + 3 * 3/4) / 10 = 3/5
    assert G == Fraction(3, 5)
    want = Fraction(3, 2) * ((5 * Fraction(3, 20)) ** 2 + (2 * Fraction(3, 5)) ** 2 + (3 * Fraction(3, 20)) ** 2) / 100
    for r in (gauc_ci_brute(y, s, u), gauc_ci_rows(y, s, u)):
        assert (r["counted"], r["left_out"]) == (3, 1) and r["gauc"] == G and r["var"] == want == Fraction(1323, 40000)      # (225 + 576 + 81) / 400 * 3 / 200
    # given weights 1, 2, 9, 1 (user 2's does not count): G = (3/4 + 0 + 3/4) / 4 = 3/8
    w = [1.0, 2.0, 9.0, 1.0]
    want = Fraction(3, 2) * (Fraction(3, 8) ** 2 + (2 * Fraction(3, 8)) ** 2 + Fraction(3, 8) ** 2) / 16
    for r in (gauc_ci_brute(y, s, u, w), gauc_ci_rows(y, s, u, w)):
        assert r["gauc"] == Fraction(3, 8) and r["var"] == want
    # paired with the scores of user 1 turned round: B = (3/4, 1, 3/4), differences (0, -1, 0), delta = -2/10
    sb = s.copy()
    sb[5:7] = [0.7, 0.2]
    want = Fraction(3, 2) * ((5 * Fraction(1, 5)) ** 2 + (2 * Fraction(-4, 5)) ** 2 + (3 * Fraction(1, 5)) ** 2) / 100
    for r in (gauc_ci_brute(y, s, u, None, sb), gauc_ci_rows(y, s, u, None, sb)):
        assert r["gauc_b"] == Fraction(4, 5) and r["delta"] == Fraction(-1, 5) and r["var_delta"] == want
    assert gauc_ci_rows(y, s, u, None, sb)["abs"] > 0 and gauc_ci_rows(y, s, u, None, sb)["abs_delta"] > 0


def test_paired_gauc_with_itself_and_with_a_monotone_transform():
    rng = np.random.default_rng(11)
    n = 200
    s = np.round(rng.random(n), 1).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.int16)
    u = rng.integers(0, 12, size=n)
    mono = (np.float32(3.0) * s + np.float32(1.0)) ** 3                             # strictly increasing on [0, 1] in float32
    assert len(np.unique(mono)) == len(np.unique(s))
    for sb in (s, s.copy(), mono):
        for r in (gauc_ci_rows(y, s, u, None, sb), gauc_ci_brute(y, s, u, None, sb)):
            assert r["delta"] == 0 and r["var_delta"] == 0 and r["gauc_b"] == r["gauc"] and r["var_b"] == r["var"] and r["var"] > 0
    rev = gauc_ci_rows(y, s, u, None, -s)
    assert rev["gauc_b"] == 1 - rev["gauc"] and rev["delta"] == 2 * rev["gauc"] - 1 and rev["var_delta"] == 4 * rev["var"]


def test_fewer_than_two_counted_users_have_no_variance():
    s = np.array([0.3, 0.7, 0.5, 0.5, 0.1], dtype=np.float32)
    for f in (gauc_ci_rows, gauc_ci_brute):
        r = f([0, 1, 1, 1, 0], s, [0, 0, 1, 1, 2], None, -s)                     # K = 1
        assert r["counted"] == 1 and r["left_out"] == 2 and r["gauc"] == 1 and r["gauc_b"] == 0 and r["delta"] == 1
        assert r["var"] is None and r["var_b"] is None and r["var_delta"] is None
        r = f([1, 1, 0, 0, 0], s, [0, 0, 1, 1, 2], None, s)                          # K = 0
        assert r["counted"] == 0 and r["left_out"] == 3 and all(r[k] is None for k in GAUC_KEYS)
        r = f([0, 1, 1, 0, 0], s, [0, 0, 1, 1, 2])                                   # K = 2
        assert r["counted"] == 2 and r["var"] is not None and "delta" not in r
    segs = gauc_ci_exact([0, 1, 1, 0], s[:4], [0, 0, 1, 1], [0, 0, 2, 2], 3)         # domain 1 empty
    assert [g["counted"] for g in segs] == [1, 0, 1, 2] and segs[1]["gauc"] is None and segs[0]["var"] is None
    assert segs[3]["gauc"] == Fraction(3, 4) and segs[3]["var"] == Fraction(1, 16)   # A = (1, 1/2), w = (2, 2): 2 * (1/4 + 1/4) / 16


def test_the_worked_loss_example():
    # terms: -log(0.5), -log(1 - 0.25) = -log(0.75), -log(0.5), -log(0.5): all four arguments are exact in float32
    y, p = [1, 0, 0, 1], np.array([0.5, 0.25, 0.5, 0.5], dtype=np.float32)
    a, b = math.log(2.0), -math.log(0.75)
    assert loss_terms(y, p) == [a, b, a, a]
    r = loss_ci_rows(y, p)
    mean = math.fsum([a, b, a, a]) / 4
    assert r["rows"] == 4 and r["P"] == 2 and r["loss"] == mean
    assert r["var"] == math.fsum([(a - mean) ** 2] * 3 + [(b - mean) ** 2]) / 12
    assert abs(r["var"] - (a - b) ** 2 / 16) <= 1e-15 * r["var"]                     # 3 (x/4)^2 + (3x/4)^2 = 12 x^2 / 16, over 12
    # float32 arithmetic of the clip: 1 - p is rounded to float32 BEFORE the clip, and both ends clip
    eps = 2.0 ** -23
    t = loss_terms([0, 1, 0, 1, 1, 0], np.array([1.0, 0.0, 1e-10, 1.0, -0.0, -0.0], dtype=np.float32))
    assert t[0] == -math.log(eps) and t[1] == -math.log(eps) and t[4] == t[1]
    assert t[2] == -math.log(1.0 - eps) and t[3] == t[2] and t[5] == t[2]            # 1 - 1e-10 rounds to 1 in float32, then clips
    # paired: the differences decide, not the two variances
    q = np.array([0.5, 0.25, 0.5, 0.25], dtype=np.float32)
    r = loss_ci_rows(y, p, q)
    d = [0.0, 0.0, 0.0, math.log(2.0) - math.log(4.0)]
    dbar = math.fsum(d) / 4
    assert r["delta"] == r["loss"] - r["loss_b"] and r["var_delta"] == math.fsum((v - dbar) ** 2 for v in d) / 12
    same = loss_ci_rows(y, p, p.copy())
    assert same["delta"] == 0.0 and same["var_delta"] == 0.0 and same["var_b"] == same["var"] > 0


def test_loss_figures_are_none_for_an_empty_or_single_class_segment():
    p = np.array([0.3, 0.7, 0.5, 0.5], dtype=np.float32)
    for y in ([0] * 4, [1] * 4):
        r = loss_ci_rows(y, p, p)
        assert all(r[k] is None for k in ("loss", "var", "loss_b", "var_b", "delta", "var_delta")) and r["rows"] == 4
    segs = loss_ci_exact([0, 1, 1, 1], p, None, [0, 0, 2, 2], 3)                     # domain 1 empty, domain 2 one class
    assert [g["rows"] for g in segs] == [2, 0, 2, 4] and [g["P"] for g in segs] == [1, 0, 2, 3]
    assert segs[1]["loss"] is None and segs[2]["var"] is None and segs[0]["var"] is not None and segs[3]["loss"] is not None
    assert loss_ci_rows([1], p[:1])["loss"] is None                                  # a single row is a single class


def test_eval_loss_ci_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, 256-byte aligned, never dereferenced on the host
    big = 1 << 40

    def call(pred_a=p, pred_b=p, label=p, domain=p, ld=1, n=10, n_domain=3, out=p, counts=p, ws=p, ws_bytes=big):
        return lib.cdc_eval_loss_ci(pred_a, pred_b, label, domain, ld, n, n_domain, out, counts, None, ws, ws_bytes, None)

    for kw in ({"pred_a": None}, {"label": None}, {"out": None}, {"counts": None}, {"ws": None}):
        assert call(**kw) == -1 and b"eval_loss_ci: null pointer" in lib.cdc_last_error(), kw
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    assert call(n=0) == -1 and call(n=-5) == -1 and call(n_domain=0) == -1 and call(n_domain=-1) == -1 and call(n_domain=1 << 20) == -1
    assert b"bad sizes" in lib.cdc_last_error()
    assert call(ld=-1) == -1
    assert call(n=1 << 31) == -2 and b"2^31" in lib.cdc_last_error()                # CDC_E_TOOBIG
    assert call(n=1 << 40, pred_b=None) == -2
    assert call(ws_bytes=1024) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws_bytes=1024, pred_b=None) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    f = lib.cdc_eval_loss_ci_workspace_bytes
    assert f(0, 3, 0) == 0 and f(10, 0, 1) == 0 and f(1 << 31, 3, 0) == 0 and f(10, 1 << 20, 0) == 0 and f(-1, 1, 1) == 0


def test_eval_gauc_ci_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)
    big = 1 << 40

    def call(pred_a=p, pred_b=p, label=p, user=p, ld_user=1, n_user=100, domain=p, ld=1, n_domain=3, w=None, n=10, out=p, counts=p, ws=p,
             ws_bytes=big):
        return lib.cdc_eval_gauc_ci(pred_a, pred_b, label, user, ld_user, n_user, domain, ld, n_domain, w, n, out, counts, None, ws,
                                    ws_bytes, None)

    for kw in ({"pred_a": None}, {"label": None}, {"user": None}, {"out": None}, {"counts": None}, {"ws": None}):
        assert call(**kw) == -1 and b"eval_gauc_ci: null pointer" in lib.cdc_last_error(), kw
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    for kw in ({"n": 0}, {"n": -5}, {"n_domain": 0}, {"n_domain": 1 << 20}, {"n_user": 0}, {"n_user": -3}, {"ld_user": -1}, {"ld": -1}):
        assert call(**kw) == -1 and b"bad sizes" in lib.cdc_last_error(), kw
    assert call(n=1 << 31) == -2 and b"2^31" in lib.cdc_last_error()                # CDC_E_TOOBIG
    assert call(n=1 << 40, pred_b=None) == -2
    assert call(n_user=(1 << 30) + 1) == -1 and b"exceed 2^32" in lib.cdc_last_error()       # 4 * n_user > 2^32
    assert call(n_user=1 << 33, n_domain=1, domain=None) == -1 and b"exceed 2^32" in lib.cdc_last_error()
    assert call(ws_bytes=1024) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws_bytes=1024, pred_b=None) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    f = lib.cdc_eval_gauc_ci_workspace_bytes
    assert f(0, 3, 100, 0) == 0 and f(10, 0, 100, 1) == 0 and f(1 << 31, 3, 100, 0) == 0 and f(10, 1 << 20, 100, 0) == 0
    assert f(10, 3, 0, 0) == 0 and f(10, 3, (1 << 30) + 1, 1) == 0


def test_ctypes_signatures_match_the_header():
    from cdcmdr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdcmdr.h")).read(), flags=re.S)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int32}
    for name in ("cdc_eval_loss_ci_workspace_bytes", "cdc_eval_loss_ci", "cdc_eval_gauc_ci_workspace_bytes", "cdc_eval_gauc_ci"):
        m = re.search(rf"(\w+)\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, name
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in (x.strip() for x in m.group(2).split(","))]
        res, args = _lib._SIGNATURES[name]
        assert res is ctype[m.group(1)] and args == want, (name, args, want)
    assert len(_lib._SIGNATURES["cdc_eval_loss_ci"][1]) == 13 and len(_lib._SIGNATURES["cdc_eval_gauc_ci"][1]) == 17


def test_host_side_of_the_new_calls():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import Evaluator, GaucCI, GaucCIPaired, LossCI, LossCIPaired, eval_gauc_ci, eval_loss_ci
    pred, label, user = torch.rand(4), torch.zeros(4, dtype=torch.int16), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.HipExtensionError):                                     # no CPU fallback
        eval_loss_ci(pred, label)
    with pytest.raises(_lib.HipExtensionError):
        eval_loss_ci(pred, label, pred_b=pred)
    with pytest.raises(_lib.HipExtensionError):
        eval_gauc_ci(pred, label, user, 5)
    with pytest.raises(_lib.HipExtensionError):
        eval_gauc_ci(pred, label, user, 5, pred_b=pred)
    with pytest.raises(ValueError, match="exceed 2\\^32"):
        eval_gauc_ci(pred, label, user, 1 << 31, n_domain=3)
    assert LossCI._fields == ("loss", "var", "rows", "positives")
    assert LossCIPaired._fields == ("loss", "var", "rows", "positives", "loss_b", "var_b", "delta", "var_delta")
    assert GaucCI._fields == ("gauc", "var", "counted", "left_out")
    assert GaucCIPaired._fields == ("gauc", "var", "counted", "left_out", "gauc_b", "var_b", "delta", "var_delta")
    ev = Evaluator(None)
    assert ev.loss_ci is False and ev.gauc_ci is False
    ev = Evaluator(None, loss_ci=True, gauc_ci=True, user_idx=2, n_user=10)
    assert ev.loss_ci is True and ev.gauc_ci is True
    with pytest.raises(ValueError, match="gauc_ci needs user_idx"):
        Evaluator(None, gauc_ci=True)
    assert Evaluator(None, loss_ci=True).gauc_ci is False                            # loss_ci needs no user column
