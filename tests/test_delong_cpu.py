"""DeLong's AUC variance without a GPU: the two exact forms of tests/delong_exact.py against each other and against hand-computed
cases, the argument checks of cdc_eval_auc_delong (they come before anything touches a device), and the host side of
eval_auc_ci / Evaluator."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from delong_exact import delong_brute, delong_exact, delong_rows, int_sum_sq, placements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("auc", "var", "auc_b", "var_b", "delta", "var_delta")


@pytest.mark.parametrize("n,levels,seed", [(2, 2, 0), (7, 2, 1), (40, 3, 2), (120, 5, 3), (300, 5, 4), (300, 1000, 5)])
def test_brute_force_equals_the_sorted_form(n, levels, seed):
    rng = np.random.default_rng(seed)
    s = (rng.integers(0, levels, size=n) / levels).astype(np.float32)              # heavy ties
    sb = np.where(rng.random(n) < 0.3, (rng.integers(0, levels, size=n) / levels).astype(np.float32), s)
    s[: n // 3][s[: n // 3] == 0] = -0.0                                            # signed zeros tie
    y = (rng.random(n) < 0.4).astype(np.int16)
    a, b = delong_brute(y, s, sb), delong_rows(y, s, sb)
    for k in KEYS:
        assert a[k] == b[k], (k, a[k], b[k])
    u = delong_brute(y, s)
    assert u["auc"] == a["auc"] and u["var"] == a["var"] and sorted(u) == ["auc", "var"]


def test_the_worked_example():
    # positives {0.9, 0.4}, negatives {0.5, 0.1, 0.4}
    y = [1, 0, 1, 0, 0]
    s = np.array([0.9, 0.5, 0.4, 0.1, 0.4], dtype=np.float32)
    a, c = placements(y, s)
    assert a.tolist() == [6, 3] and c.tolist() == [2, 4, 3]
    r = delong_rows(y, s)
    assert r["sums"] == (9, 45, 9, 29) and (r["P"], r["N"]) == (2, 3)
    assert r["auc"] == Fraction(3, 4) and r["var"] == Fraction(1, 12)
    P, N = 2, 3
    assert Fraction(P * 45 - 81, P * (P - 1) * 4 * N * N) == Fraction(1, 8)         # S10
    assert Fraction(N * 29 - 81, N * (N - 1) * 4 * P * P) == Fraction(1, 16)        # S01
    assert delong_brute(y, s) == {"auc": Fraction(3, 4), "var": Fraction(1, 12)}


def test_degenerate_orders():
    y = np.array([0] * 9 + [1] * 6)
    sep = np.arange(15, dtype=np.float32)                                           # perfectly separated
    for r in (delong_rows(y, sep), delong_brute(y, sep)):
        assert r["auc"] == 1 and r["var"] == 0
    for r in (delong_rows(y, -sep), delong_brute(y, -sep)):
        assert r["auc"] == 0 and r["var"] == 0
    tied = np.full(15, 0.25, dtype=np.float32)
    tied[::2] = 0.25
    for r in (delong_rows(y, tied), delong_brute(y, tied)):
        assert r["auc"] == Fraction(1, 2) and r["var"] == 0
    zeros = np.array([0.0, -0.0] * 8, dtype=np.float32)[:15]
    assert delong_rows(y, zeros)["auc"] == Fraction(1, 2) and delong_rows(y, zeros)["var"] == 0


def test_a_single_row_of_a_class_has_an_auc_and_no_variance():
    s = np.array([0.3, 0.7, 0.5, 0.5, 0.1], dtype=np.float32)
    for y in ([0, 1, 0, 0, 0], [1, 0, 1, 1, 1]):
        for r in (delong_rows(y, s, s[::-1].copy()), delong_brute(y, s, s[::-1].copy())):
            assert r["auc"] is not None and r["delta"] is not None
            assert r["var"] is None and r["var_b"] is None and r["var_delta"] is None
    assert delong_rows([0, 1, 0, 0, 0], s)["auc"] == 1 and delong_rows([1, 0, 1, 1, 1], s)["auc"] == 0
    for y in ([0] * 5, [1] * 5):
        r = delong_rows(y, s, s)
        assert all(r[k] is None for k in KEYS) and delong_brute(y, s, s)["delta"] is None
    segs = delong_exact([0, 1, 1, 0], s[:4], None, [0, 0, 2, 2], 3)                  # domain 1 empty
    assert [g["rows"] for g in segs] == [2, 0, 2, 4] and segs[1]["auc"] is None and segs[3]["var"] is not None


def test_paired_with_itself_and_with_a_monotone_transform():
    rng = np.random.default_rng(11)
    n = 200
    s = np.round(rng.random(n), 1).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.int16)
    mono = (np.float32(3.0) * s + np.float32(1.0)) ** 3                             # strictly increasing on [0, 1] in float32
    assert len(np.unique(mono)) == len(np.unique(s))
    for sb in (s, s.copy(), mono):
        for r in (delong_rows(y, s, sb), delong_brute(y, s, sb)):
            assert r["delta"] == 0 and r["var_delta"] == 0 and r["auc_b"] == r["auc"] and r["var_b"] == r["var"] and r["var"] > 0
    rev = delong_rows(y, s, -s)
    assert rev["auc_b"] == 1 - rev["auc"] and rev["delta"] == 2 * rev["auc"] - 1 and rev["var_delta"] == 4 * rev["var"]


def test_integer_sums_do_not_overflow():
    x = np.full(3 * (1 << 20) + 5, (1 << 32) - 2, dtype=np.int64)
    x[::2] *= -1
    assert int_sum_sq(x) == len(x) * ((1 << 32) - 2) ** 2 and int_sum_sq(x) > 1 << 85


def test_eval_auc_delong_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, 256-byte aligned, never dereferenced on the host
    big = 1 << 40

    def call(pred_a=p, pred_b=p, label=p, domain=p, ld=1, n=10, n_domain=3, out=p, counts=p, ws=p, ws_bytes=big):
        return lib.cdc_eval_auc_delong(pred_a, pred_b, label, domain, ld, n, n_domain, out, counts, None, ws, ws_bytes, None)

    for kw in ({"pred_a": None}, {"label": None}, {"out": None}, {"counts": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.cdc_last_error(), kw
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    assert call(n=0) == -1 and call(n=-5) == -1 and call(n_domain=0) == -1 and call(n_domain=-1) == -1 and call(n_domain=1 << 20) == -1
    assert b"bad sizes" in lib.cdc_last_error()
    assert call(ld=-1) == -1
    assert call(n=1 << 31) == -2 and b"2^31" in lib.cdc_last_error()                # CDC_E_TOOBIG
    assert call(n=1 << 40, pred_b=None) == -2
    assert call(ws_bytes=1024) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws_bytes=1024, pred_b=None) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    f = lib.cdc_eval_auc_delong_workspace_bytes
    assert f(0, 3, 0) == 0 and f(10, 0, 1) == 0 and f(1 << 31, 3, 0) == 0 and f(10, 1 << 20, 0) == 0


def test_ctypes_signature_matches_the_header():
    from cdcmdr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdcmdr.h")).read(), flags=re.S)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int32}
    for name in ("cdc_eval_auc_delong_workspace_bytes", "cdc_eval_auc_delong"):
        m = re.search(rf"(\w+)\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, name
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in (x.strip() for x in m.group(2).split(","))]
        res, args = _lib._SIGNATURES[name]
        assert res is ctype[m.group(1)] and args == want, (name, args, want)
    assert len(_lib._SIGNATURES["cdc_eval_auc_delong"][1]) == 13


def test_eval_auc_ci_host_side():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import AucCI, AucCIPaired, Evaluator, _z, eval_auc_ci
    pred, label = torch.rand(4), torch.zeros(4, dtype=torch.int16)
    with pytest.raises(_lib.HipExtensionError):                                     # no CPU fallback
        eval_auc_ci(pred, label)
    with pytest.raises(_lib.HipExtensionError):
        eval_auc_ci(pred, label, pred_b=pred)
    assert AucCI._fields == ("auc", "var", "rows", "positives")
    assert AucCIPaired._fields == ("auc", "var", "rows", "positives", "auc_b", "var_b", "delta", "var_delta")
    assert math.isnan(_z(0.0, 0.0)) and _z(1e-4, 0.0) == math.inf and _z(-1e-4, 0.0) == -math.inf and _z(1.0, 0.5) == 2.0
    assert math.isnan(_z(1.0, math.nan)) and math.isnan(_z(math.nan, 1.0))
    assert Evaluator(None).auc_ci is False and Evaluator(None, auc_ci=True).auc_ci is True
    with pytest.raises(ValueError, match="precision"):
        Evaluator(None, precision="fp16")
