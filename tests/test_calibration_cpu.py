"""Calibration figures without a GPU: the exact helper tests/calibration_exact.py against its own row-by-row form, against plain
float64 numpy on the unquantised predictions, against sklearn and against hand-computed cases; the argument checks of
cdc_eval_calibration (they come before anything touches a device) and the host side of eval_calibration / Evaluator.

The float64 bounds are derived.  A prediction enters the helper as q / 2^32 with |q / 2^32 - p| <= 2^-33 (zero for p >= 2^-8, where
the float32 has no bit below 2^-32), the bins are the same on both sides (floor(p K) is exact in float64, the sort is the same), so
  mean_pred, ece, mce   a mean of, or a sum over bins of means of, per-row differences <= 2^-33: <= 2^-33
  brier                 |a^2 - b^2| = |a - b| |a + b| <= 2^-33 * 2 = 2^-32 per row, hence for the mean
  pcoc                  sum of the differences over the positives' count: <= (rows / positives) 2^-33
and the float64 side adds a few roundings (its sums are math.fsum's, rounded once): 8 * 2^-53 relative is allowed for them."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from calibration_exact import (ONE, SEGMENT_FIELDS, TABLE_FIELDS, calibration_exact, calibration_rows, calibration_rows_slow,
                               quantise, width_bins)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _ctr_like(rng, n):
    """most mass below 0.1, many values below 2^-8 (where q is rounded), a tie run, and the ends of the range"""
    p = (rng.random(n) ** 4).astype(np.float32)
    p[rng.random(n) < 0.1] = np.float32(0.03125)
    p[:4] = [0.0, 1.0, 2.0 ** -40, 1.0 - 2.0 ** -24][:min(n, 4)]
    y = (rng.random(n) < 0.05 + 0.5 * p).astype(np.int16)
    return p, y


@pytest.mark.parametrize("n,K,seed", [(0, 3, 0), (1, 1, 1), (1, 4, 2), (5, 10, 3), (40, 7, 4), (200, 16, 5), (300, 1024, 6)])
def test_the_numpy_form_equals_the_row_by_row_form(n, K, seed):
    rng = np.random.default_rng(seed)
    p, y = _ctr_like(rng, n)
    p[n // 2:] = np.round(p[n // 2:], 1)                                             # heavy ties, some on bin edges
    p[: n // 3][p[: n // 3] == 0] = -0.0
    a, b = calibration_rows(y, p, K), calibration_rows_slow(y, p, K)
    assert sorted(a) == sorted(b)
    for k in ("rows", "positives", "sum_q") + SEGMENT_FIELDS:
        assert a[k] == b[k], (k, a[k], b[k])
    for t in ("table", "table_q"):
        for f in TABLE_FIELDS:
            got, want = a[t][f], b[t][f]
            assert len(got) == len(want) == K
            if f.startswith("pred_m"):                                                # float32: the same bits
                assert [None if v is None else np.float32(v).view(np.int32) for v in got] == \
                       [None if v is None else np.float32(v).view(np.int32) for v in want], (t, f)
            else:
                assert got == want, (t, f, got, want)


def test_quantisation_and_bins_against_fractions():
    rng = np.random.default_rng(7)
    p = np.concatenate([rng.random(500).astype(np.float32), (rng.random(500) * 2.0 ** -9).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 2.0 ** -33, 2.0 ** -34, 3 * 2.0 ** -34, 1e-45, 1.0 - 2.0 ** -24, 0.1, 0.3, 0.5, 0.7],
                                 dtype=np.float32), (np.arange(17) / 16).astype(np.float32), (np.arange(11) / np.float32(10)).astype(np.float32)])
    q = quantise(p)
    assert q.min() == 0 and q.max() == ONE
    for pi, qi in zip(p, q):
        f = Fraction(float(pi))
        assert int(qi) == round(f * ONE)                                              # half to even: 2^-33 -> 0, 3 * 2^-34 -> 1
        assert abs(Fraction(int(qi), ONE) - f) <= Fraction(1, 1 << 33)
        if f >= Fraction(1, 256):
            assert Fraction(int(qi), ONE) == f                                        # exact from 2^-8 up
    assert int(quantise([2.0 ** -33])[0]) == 0 and int(quantise([3 * 2.0 ** -34])[0]) == 1 and int(quantise([2.0 ** -40])[0]) == 0
    for K in (1, 2, 3, 10, 15, 16, 1000, 1024):
        assert width_bins(p, K).tolist() == [min(K - 1, int(Fraction(float(v)) * K)) for v in p], K


@pytest.mark.parametrize("seed", range(20))
def test_against_float64_numpy_on_the_unquantised_predictions(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(50, 3000))
    p, y = _ctr_like(rng, n)
    order = np.lexsort((y, p))
    p64, y64 = p[order].astype(np.float64), y[order].astype(np.float64)
    P = int(y.sum())
    for K in (1, 2, 10, 15, 1024):
        r = calibration_rows(y, p, K)

        def close(name, got, want, bound):
            err = abs(float(got) - want)
            print(seed, K, name, "helper", float(got), "float64", want, "difference", err, "bound", bound)
            assert err <= bound + 8 * U * abs(want), (seed, K, name, float(got), want, err, bound)

        close("mean_pred", r["mean_pred"], math.fsum(p64) / n, 2.0 ** -33)
        close("ctr", r["ctr"], P / n, 0.0)
        close("brier", r["brier"], math.fsum((p64 - y64) ** 2) / n, 2.0 ** -32)
        if P:
            close("pcoc", r["pcoc"], math.fsum(p64) / P, n / P * 2.0 ** -33)
        bw = np.minimum(np.floor(p64 * K), K - 1).astype(np.int64)
        for name, bins in (("", [np.flatnonzero(bw == b) for b in range(K)]),
                           ("_q", [np.arange((b * n) // K, ((b + 1) * n) // K) for b in range(K)])):
            gaps = [(abs(math.fsum(p64[ix]) - y64[ix].sum()), len(ix)) for ix in bins if len(ix)]
            close("ece" + name, r["ece" + name], math.fsum(g for g, _ in gaps) / n, 2.0 ** -33)
            close("mce" + name, r["mce" + name], max(g / c for g, c in gaps), 2.0 ** -33)
            t = r["table" + name]
            assert t["count"] == [len(ix) for ix in bins] and sum(t["count"]) == n and sum(t["positives"]) == P


def test_against_sklearn():
    from sklearn.calibration import calibration_curve
    from sklearn.metrics import brier_score_loss
    rng = np.random.default_rng(11)
    n = 4000
    p, y = _ctr_like(rng, n)
    r = calibration_rows(y, p, 10)
    want = brier_score_loss(y.astype(np.int64), p.astype(np.float64))
    assert abs(float(r["brier"]) - want) <= 2.0 ** -32 + 16 * U * want, (float(r["brier"]), want)
    # sklearn compares with float edges (a prediction ON an edge goes to the bin below): keep the predictions away from them
    for K in (4, 10, 15):
        b = rng.integers(0, K, size=n)
        b[b == 3] = 1                                                                 # an empty bin: sklearn leaves it out
        p = ((b + 0.1 + 0.8 * rng.random(n)) / K).astype(np.float32)
        y = (rng.random(n) < p).astype(np.int64)
        assert np.array_equal(width_bins(p, K), b)
        prob_true, prob_pred = calibration_curve(y, p.astype(np.float64), n_bins=K, strategy="uniform")
        t = calibration_rows(y, p, K)["table"]
        keep = [i for i in range(K) if t["count"][i]]
        assert len(keep) == K - 1 == len(prob_true) and t["count"][3] == 0 and t["mean_pred"][3] is None
        for j, i in enumerate(keep):
            assert abs(float(t["pos_rate"][i]) - prob_true[j]) <= 4 * U * prob_true[j], (K, i)
            assert abs(float(t["mean_pred"][i]) - prob_pred[j]) <= 2.0 ** -33 + 16 * U * prob_pred[j], (K, i)


def test_the_worked_example():
    """Five rows with dyadic predictions (q / 2^32 == p): every figure by hand."""
    p = np.array([0.25, 1.0, 0.125, 0.75, 0.25], dtype=np.float32)
    y = [1, 1, 0, 1, 0]
    for fn in (calibration_rows, calibration_rows_slow):
        r = fn(y, p, 2)
        assert (r["rows"], r["positives"], r["sum_q"]) == (5, 3, 19 * ONE // 8)
        assert r["mean_pred"] == Fraction(19, 40) and r["ctr"] == Fraction(3, 5) and r["pcoc"] == Fraction(19, 24)
        assert r["brier"] == Fraction(9, 64)                                          # (9/16 + 0 + 1/64 + 1/16 + 1/16) / 5
        # equal width: [0, 0.5) holds 0.125, 0.25, 0.25 (one positive), [0.5, 1] holds 0.75, 1.0 (both positive)
        t = r["table"]
        assert t["count"] == [3, 2] and t["positives"] == [1, 2]
        assert t["mean_pred"] == [Fraction(5, 24), Fraction(7, 8)] and t["pos_rate"] == [Fraction(1, 3), Fraction(1)]
        assert [float(v) for v in t["pred_min"]] == [0.125, 0.75] and [float(v) for v in t["pred_max"]] == [0.25, 1.0]
        assert r["ece"] == Fraction(1, 8) and r["mce"] == Fraction(1, 8)              # (|5/8 - 1| + |7/4 - 2|) / 5; 3/8 / 3 = 1/4 / 2
        # equal mass: sorted by (p, y) the rows are (1/8, 0) (1/4, 0) | (1/4, 1) (3/4, 1) (1, 1): the tie at 1/4 is cut by the bound
        t = r["table_q"]
        assert t["count"] == [2, 3] and t["positives"] == [0, 3]
        assert t["mean_pred"] == [Fraction(3, 16), Fraction(2, 3)] and t["pos_rate"] == [Fraction(0), Fraction(1)]
        assert [float(v) for v in t["pred_min"]] == [0.125, 0.25] and [float(v) for v in t["pred_max"]] == [0.25, 1.0]
        assert r["ece_q"] == Fraction(11, 40) and r["mce_q"] == Fraction(1, 3)        # (3/8 + |2 - 3|) / 5; max(3/16, 1/3)


def test_one_bin_fewer_rows_than_bins_and_degenerate_segments():
    rng = np.random.default_rng(13)
    p, y = _ctr_like(rng, 500)
    r = calibration_rows(y, p, 1)
    assert r["ece"] == r["ece_q"] == r["mce"] == r["mce_q"] == abs(r["mean_pred"] - r["ctr"])
    assert r["table"]["count"] == r["table_q"]["count"] == [500]
    # 3 rows, 8 bins: equal-mass bins [0,0) [0,0) [0,1) [1,1) [1,1) [1,2) [2,2) [2,3)
    r = calibration_rows([1, 0, 1], np.array([0.9, 0.2, 0.5], dtype=np.float32), 8)
    assert r["table_q"]["count"] == [0, 0, 1, 0, 0, 1, 0, 1] and r["table_q"]["positives"] == [0, 0, 0, 0, 0, 1, 0, 1]
    assert r["table"]["count"] == [0, 1, 0, 0, 1, 0, 0, 1]
    assert r["table_q"]["mean_pred"][0] is None and r["table_q"]["pred_min"][3] is None
    assert r["ece"] == r["ece_q"] and r["mce"] == r["mce_q"] == Fraction(quantise([0.5])[0], ONE)          # a bin per row: |p - y|
    # an empty and a single-class segment
    segs = calibration_exact([0, 0, 1, 1], np.array([0.5, 0.25, 0.5, 0.75], dtype=np.float32), 4, [0, 0, 2, 2], 3)
    assert [s["rows"] for s in segs] == [2, 0, 2, 4]
    assert all(segs[1][k] is None for k in SEGMENT_FIELDS) and segs[1]["table"]["count"] == [0] * 4
    assert segs[0]["pcoc"] is None and segs[0]["brier"] == Fraction(5, 32) and segs[0]["ece"] == Fraction(3, 8)
    assert segs[2]["pcoc"] == Fraction(5, 8) and segs[2]["ctr"] == 1
    # p = 1 belongs to the last bin, an edge b / K to bin b
    assert calibration_rows([1] * 3, np.array([1.0, 0.5, 0.25], dtype=np.float32), 4)["table"]["count"] == [0, 1, 1, 1]


def test_a_tie_run_of_mixed_labels_across_a_quantile_bound_does_not_depend_on_the_row_order():
    rng = np.random.default_rng(17)
    p = np.array([0.1] * 3 + [0.3] * 11 + [0.8] * 4, dtype=np.float32)              # 18 rows, 4 bins: bounds 4, 9, 13 cut the run of 0.3
    y = np.array([0, 1, 0] + [1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1] + [1, 1, 0, 1])
    base = calibration_rows(y, p, 4)
    # sorted: 0.1 x (0,0,1) | 0.3 x (0 x6, 1 x5) | 0.8 x (0,1,1,1); bins [0,4) [4,9) [9,13) [13,18)
    assert base["table_q"]["count"] == [4, 5, 4, 5] and base["table_q"]["positives"] == [1, 0, 4, 4]
    for _ in range(5):
        perm = rng.permutation(len(y))
        for fn in (calibration_rows, calibration_rows_slow):
            assert fn(y[perm], p[perm], 4) == base


def test_eval_calibration_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-null, 256-byte aligned, never dereferenced on the host
    big = 1 << 40

    def call(pred=p, label=p, domain=p, ld=1, n=10, n_domain=3, n_bins=10, seg_out=p, seg_counts=p, tab_out=p, tab_counts=p, tab_range=p,
             ws=p, ws_bytes=big):
        return lib.cdc_eval_calibration(pred, label, domain, ld, n, n_domain, n_bins, seg_out, seg_counts, tab_out, tab_counts, tab_range,
                                        None, ws, ws_bytes, None)

    for kw in ({"pred": None}, {"label": None}, {"seg_out": None}, {"seg_counts": None}, {"tab_out": None}, {"tab_counts": None},
               {"tab_range": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.cdc_last_error(), kw
    for k in (0, 1025, -1):
        assert call(n_bins=k) == -1 and b"n_bins" in lib.cdc_last_error(), k
    assert call(domain=None) == -1 and b"domain column" in lib.cdc_last_error()
    assert call(n=0) == -1 and call(n=-5) == -1 and call(n_domain=0) == -1 and call(n_domain=1 << 20) == -1
    assert b"bad sizes" in lib.cdc_last_error()
    assert call(ld=-1) == -1
    assert call(n=1 << 31) == -2 and b"2^31" in lib.cdc_last_error()                # CDC_E_TOOBIG
    assert call(ws_bytes=1024) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws_bytes=1024, n_bins=1, n_domain=1, domain=None) == -1 and b"workspace 1024 <" in lib.cdc_last_error()
    assert call(ws=C.c_void_p(4096 + 64)) == -1 and b"256-byte aligned" in lib.cdc_last_error()
    f = lib.cdc_eval_calibration_workspace_bytes
    assert f(0, 3, 10) == 0 and f(10, 0, 10) == 0 and f(1 << 31, 3, 10) == 0 and f(10, 1 << 20, 10) == 0
    assert f(10, 3, 0) == 0 and f(10, 3, 1025) == 0


def test_ctypes_signature_matches_the_header():
    from cdcmdr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdcmdr.h")).read(), flags=re.S)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int32}
    for name in ("cdc_eval_calibration_workspace_bytes", "cdc_eval_calibration"):
        m = re.search(rf"(\w+)\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, name
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in (x.strip() for x in m.group(2).split(","))]
        res, args = _lib._SIGNATURES[name]
        assert res is ctype[m.group(1)] and args == want, (name, args, want)
    assert len(_lib._SIGNATURES["cdc_eval_calibration"][1]) == 16


def test_eval_calibration_host_side():
    from cdcmdr_amd import _lib
    from cdcmdr_amd.evaluate import Calibration, CalibrationTable, Evaluator, eval_calibration
    pred, label = torch.rand(4), torch.zeros(4, dtype=torch.int16)
    with pytest.raises(_lib.HipExtensionError):                                     # no CPU fallback
        eval_calibration(pred, label)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="n_bins"):
            eval_calibration(pred, label, n_bins=k)
    assert Calibration._fields == ("rows", "positives", "mean_pred", "ctr", "pcoc", "brier", "ece", "mce", "ece_q", "mce_q", "table", "table_q")
    assert CalibrationTable._fields == TABLE_FIELDS
    assert Evaluator(None).calibration_bins == 0 and Evaluator(None, calibration=True).calibration_bins == 10
    assert Evaluator(None, calibration=15).calibration_bins == 15 and Evaluator(None, calibration=1).calibration_bins == 1
    for k in (0, 1025, -3):
        with pytest.raises(ValueError, match="calibration"):
            Evaluator(None, calibration=k)
