"""The bootstrap of the calibration figures without a device: the two reference forms of tests/calibration_boot_exact.py against
each other, the exported symbols and the argument checks of cdc_eval_calibration_bootstrap (the library loads without a GPU; nothing
is launched), and the statistical sense of the definition on two fixed data sets."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import bootstrap_exact as B
import calibration_boot_exact as CB
from calibration_exact import calibration_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_source():
    return open(os.path.join(ROOT, "causal-domain-clustering-for-multi-domain-recommendation_amd", "csrc", "metrics.hip")).read()


def rows_case(seed=5, n=4000):
    """the issue's rows case: skewed scores, clicks at 0.03 + 0.6 p"""
    rng = np.random.default_rng(seed)
    p = (rng.random(n) ** 5).astype(np.float32)
    y = (rng.random(n) < 0.03 + 0.6 * p).astype(np.int16)
    return p, y


def clustered_case(seed=6, users=400, per=10):
    """the issue's clustered case: every user shifts the click probability of all of their rows"""
    rng = np.random.default_rng(seed)
    shift = rng.normal(0.0, 0.15, users)
    user = np.repeat(np.arange(users), per).astype(np.int32)
    p = (0.2 + 0.1 * rng.random(users * per)).astype(np.float32)
    y = (rng.random(users * per) < np.clip(p + shift[user], 0.0, 1.0)).astype(np.int16)
    return p, y, user


def brier_errors(p, y, user=None):
    """analytic standard errors of the Brier score: rows independent, and linearised over clusters"""
    e = (p.astype(np.float64) - y) ** 2
    n = len(e)
    rows = e.std(ddof=1) / math.sqrt(n)
    if user is None:
        return rows, None
    g = np.bincount(user, weights=e - e.mean())
    G = len(g)
    return rows, math.sqrt(G / (G - 1) * (g ** 2).sum()) / n


def brier_spread(p, y, user, seed, n_rep=400):
    """standard deviation of the helper's Brier replicates over all rows (weights straight from the recipe: only W and SE2 enter)"""
    e = (p.astype(np.float64) - y) ** 2
    c = np.arange(len(p)) if user is None else user
    reps = []
    for r in range(n_rep):
        w = B.weights(seed, r, c)
        reps.append((w * e).sum() / w.sum())
    return float(np.std(reps, ddof=1))


@pytest.mark.parametrize("case", range(12))
def test_the_two_reference_forms_agree_exactly(case):
    rng = np.random.default_rng(100 + case)
    n = int(rng.integers(1, 40))
    K = [1, 2, 3, 7, 10, 64, 1024][case % 7]                   # K > W: a row's copies span several bins, most bins are empty
    n_domain = 1 + case % 3
    grid = rng.integers(0, 6, n) / 5.0 if case % 2 else rng.random(n)          # a coarse grid: long tie runs
    p = grid.astype(np.float32)
    y = rng.integers(0, 2, n).astype(np.int16)
    domain = rng.integers(0, n_domain, n).astype(np.int32) if n_domain > 1 else None
    cluster = rng.integers(0, max(1, n // 3), n).astype(np.int32) if case % 4 >= 2 else None
    a = CB.by_expansion(y, p, K, cluster, seed=case, n_rep=5, domain=domain, n_domain=n_domain)
    b = CB.direct(y, p, K, cluster, seed=case, n_rep=5, domain=domain, n_domain=n_domain)
    assert a == b
    split = False
    for r in range(5):
        w = CB.rep_weights(case, r, n, cluster)
        for s in a[r]:
            assert (s["W"] == 0) == (s["brier"] is None) == (s["ece"] is None) == (s["ece_q"] is None)
            assert (s["pcoc"] is None) == (s["Wp"] == 0)
        assert a[r][-1]["W"] == int(w.sum()) and a[r][-1]["Wp"] == int((w * (y != 0)).sum())
        split |= K > a[r][-1]["W"] > 0 and int(w.max()) > 1
    if K == 1024:
        assert split                                           # a row of weight > 1 lay in more bins than one


def test_weight_one_is_the_plain_calibration_and_a_split_row_is_counted_by_copies():
    p = np.array([0.1, 0.4, 0.4, 0.8, 0.9], dtype=np.float32)
    y = np.array([0, 1, 0, 1, 1], dtype=np.int16)
    want = calibration_rows(y, p, 3)
    for form in (CB.by_expansion, CB.direct):
        got = form(y, p, 3, weight_fn=B.ones)[0][-1]
        assert got["W"] == 5 and all(got[k] == want[k] for k in CB.FIGURES)
    # weights (0, 3, 0, 1, 0), K = 2: W = 4, bin 0 = two copies of row 1, bin 1 = its third copy and row 3
    fixed = lambda seed, r, c: np.array([0, 3, 0, 1, 0])
    got = CB.direct(y, p, 2, weight_fn=fixed)[0][-1]
    assert got == CB.by_expansion(y, p, 2, weight_fn=fixed)[0][-1]
    q1, q3 = (int(np.rint(float(v) * 2 ** 32)) for v in (p[1], p[3]))
    gap = abs(2 * q1 - 2 * 2 ** 32) + abs(q1 + q3 - 2 * 2 ** 32)
    assert got["W"] == 4 and got["Wp"] == 4 and got["ece_q"] == Fraction(gap, 4 * 2 ** 32)


def test_the_library_exports_the_entry_points_and_the_python_side_mirrors_the_tiles():
    from cdcmdr_amd import _lib, evaluate
    header = open(os.path.join(ROOT, "include", "cdcmdr.h")).read()
    lib = _lib.load()
    for name in ("cdc_eval_calibration_bootstrap_workspace_bytes", "cdc_eval_calibration_bootstrap"):
        assert name in _lib.exported_symbols() and re.search(rf"\b{name}\(", header)
        assert getattr(lib, name).argtypes is not None
    src = _kernel_source()
    for name in ("CALBOOT_CHUNK", "CALBOOT_REP_TILE"):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1)) == getattr(evaluate, name), name
    assert re.search(r"#define\s+CALBOOT_MAX_CELLS\s+\(1 << 22\)", src) and evaluate.CALBOOT_MAX_CELLS == 1 << 22
    assert evaluate.CalibrationBootstrap._fields == ("pcoc", "brier", "ece", "ece_q", "w_rows", "w_pos", "pcoc_b", "brier_b", "ece_b",
                                                     "ece_q_b")


def test_entry_point_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    one, ws = C.c_void_p(16), C.c_void_p(256)
    big = 1 << 40

    def call(pred=one, pred_b=None, label=one, cluster=one, ld_c=1, n_c=10, domain=one, ld_d=1, n_domain=3, n_bins=10, n=100, n_rep=8,
             seed=0, out=one, counts=one, err=None, work=ws, nbytes=big):
        return lib.cdc_eval_calibration_bootstrap(pred, pred_b, label, cluster, ld_c, n_c, domain, ld_d, n_domain, n_bins, n, n_rep, seed,
                                                  out, counts, err, work, nbytes, None)

    BADARG, TOOBIG = -1, -2
    for bad in (dict(pred=None), dict(label=None), dict(out=None), dict(counts=None), dict(work=None)):
        assert call(**bad) == BADARG and b"null pointer" in lib.cdc_last_error(), bad
    for bad in (dict(n=0), dict(n=-5), dict(n_domain=0), dict(n_domain=1 << 20), dict(ld_c=-1), dict(ld_d=-1), dict(n_c=0)):
        assert call(**bad) == BADARG and b"bad sizes" in lib.cdc_last_error(), bad
    for n_bins in (0, -1, 1025):
        assert call(n_bins=n_bins) == BADARG and b"n_bins" in lib.cdc_last_error()
    for n_rep in (0, -1, 4097):
        assert call(n_rep=n_rep) == BADARG and b"n_rep" in lib.cdc_last_error()
    assert call(domain=None) == BADARG and b"needs the domain column" in lib.cdc_last_error()
    assert call(n=1 << 28) == TOOBIG and b"2^28" in lib.cdc_last_error()
    assert call(n_rep=4096, n_bins=1024, n_domain=1) == TOOBIG and b"cells exceed 2^22" in lib.cdc_last_error()
    assert call(n_rep=2049, n_bins=1024, n_domain=1) == TOOBIG                 # 2049 * 2 * 1024 = 2^22 + 2048
    assert call(work=C.c_void_p(264)) == BADARG and b"256-byte aligned" in lib.cdc_last_error()
    assert call(nbytes=1024) == BADARG and b"workspace" in lib.cdc_last_error()
    assert call(cluster=None, nbytes=1024) == BADARG and b"workspace" in lib.cdc_last_error()
    # the size query: positive for a valid shape (plain arithmetic: no device is asked), 0 for every refused one
    q = lib.cdc_eval_calibration_bootstrap_workspace_bytes
    assert q(100, 3, 10, 8, 0) > 0 and q(100, 3, 10, 8, 1) > 0 and q(500000, 50, 10, 200, 1) > 0
    assert q(100, 1, 1024, 2048, 0) > 0                                       # exactly 2^22 cells
    assert q(100, 3, 10, 8, 0) % 256 == 0
    for refused in ((0, 3, 10, 8), (-1, 3, 10, 8), (1 << 28, 3, 10, 8), (100, 0, 10, 8), (100, 1 << 20, 10, 8), (100, 3, 0, 8),
                    (100, 3, 1025, 8), (100, 3, 10, 0), (100, 3, 10, 4097), (100, 1, 1024, 2049), (100, 3, 1024, 4096)):
        assert q(*refused, 0) == 0 and q(*refused, 1) == 0, refused
    # the wrapper's own checks come before any device work as well
    from cdcmdr_amd.evaluate import eval_calibration_bootstrap
    p, y = torch.zeros(4), torch.zeros(4, dtype=torch.int16)
    with pytest.raises(ValueError, match="n_rep"):
        eval_calibration_bootstrap(p, y, n_rep=0)
    with pytest.raises(ValueError, match="n_bins"):
        eval_calibration_bootstrap(p, y, n_bins=1025)
    with pytest.raises(ValueError, match="CALBOOT_MAX_CELLS"):
        eval_calibration_bootstrap(p, y, n_bins=1024, n_rep=4096)
    with pytest.raises(ValueError, match="n_cluster"):
        eval_calibration_bootstrap(p, y, cluster=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.HipExtensionError):
        eval_calibration_bootstrap(p, y)


def test_evaluator_calibration_ci_needs_calibration_and_bootstrap():
    from cdcmdr_amd.evaluate import Evaluator
    for kw in (dict(), dict(calibration=True), dict(bootstrap=50)):
        with pytest.raises(ValueError, match="calibration_ci needs calibration"):
            Evaluator(None, mode="single", calibration_ci=True, **kw)
    ev = Evaluator(None, mode="single", calibration=5, bootstrap=50, calibration_ci=True)
    assert ev.calibration_ci and ev.calibration_bins == 5 and ev.bootstrap == 50
    assert Evaluator(None, mode="single").calibration_ci is False


def test_brier_replicates_spread_like_the_analytic_errors():
    """Rows case: sd of the replicates against std((p - y)^2) / sqrt(n); clustered case: against the cluster-linearised error, which
    the row formula understates.  400 replicates: the sd of a standard deviation is 1 / sqrt(2 * 399) = 3.5 %, +-15 % is 4 sigma."""
    p, y = rows_case()
    rows_se, _ = brier_errors(p, y)
    ratio_rows = brier_spread(p, y, None, seed=7) / rows_se
    # the helper's own replicates (quantised predictions, the full figure set) give the same spread
    res = CB.direct(y, p, 10, seed=7, n_rep=40)
    e = (p.astype(np.float64) - y) ** 2
    for r in (0, 39):
        w = B.weights(7, r, np.arange(len(p)))
        assert abs(float(res[r][-1]["brier"]) - (w * e).sum() / w.sum()) < 1e-9
    pc, yc, user = clustered_case()
    rows_c, clustered_se = brier_errors(pc, yc, user)
    spread_c = brier_spread(pc, yc, user, seed=7)
    print("rows case: ratio", ratio_rows, "clustered case: against clustered", spread_c / clustered_se, "against rows", spread_c / rows_c)
    assert abs(ratio_rows - 1) <= 0.15
    assert abs(spread_c / clustered_se - 1) <= 0.15
    assert spread_c >= 1.2 * rows_c
