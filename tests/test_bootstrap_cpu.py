"""The clustered bootstrap without a device: the weight recipe, the two reference forms of tests/bootstrap_exact.py against each
other and against the unweighted helpers, `summarize_bootstrap` on CPU tensors, and the argument checks of cdc_eval_bootstrap
(the library loads without a GPU; nothing is launched)."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import bootstrap_exact as B
from delong_exact import delong_exact
from gauc_ci_exact import gauc_ci_exact
from loss_ci_exact import loss_ci_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISSUE_T = [0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21,
           0xffffffd4, 0xfffffffc]


def _kernel_source():
    return open(os.path.join(ROOT, "causal-domain-clustering-for-multi-domain-recommendation_amd", "csrc", "metrics.hip")).read()


def test_thresholds_equal_the_decimal_recomputation_and_the_kernel_source():
    assert B.thresholds() == ISSUE_T == B.T
    body = re.search(r"uint32_t boot_weight\(.*?\n}", _kernel_source(), flags=re.S).group(0)
    assert [int(h, 16) for h in re.findall(r"u >= (0x[0-9a-f]{8})u", body)] == ISSUE_T
    # the cap: the 13th threshold would be 2^32 itself in 32 bits' resolution
    assert ISSUE_T == sorted(ISSUE_T) and ISSUE_T[-1] < 1 << 32


def test_the_python_side_mirrors_the_kernel_tiles():
    from cdcmdr_amd import evaluate
    src = _kernel_source()
    for name in ("BOOT_CHUNK", "BOOT_REP_TILE", "BOOT_MAX_REP"):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1)) == getattr(evaluate, name), name
    assert evaluate.BOOT_MAX_ROWS == (1 << 28) - 1


def test_weights_are_a_fixed_poisson_like_function():
    # spot values of the pure-integer form pin the recipe; the vectorised form must agree with it everywhere it is tried
    assert B.mix(0) == 0 and B.mix(1) == 0x5692161D100B05E5
    for seed, r in [(0, 0), (0, 1), (12345, 7), ((1 << 64) - 1, 4095)]:
        c = np.r_[np.arange(50), [2 ** 31 - 1, 2 ** 28, 99999]]
        assert B.weights(seed, r, c).tolist() == [B.weight(seed, r, int(k)) for k in c]
    w = np.concatenate([B.weights(0, r, np.arange(1000)) for r in range(100)])     # 10^5 (replicate, cluster) pairs
    N = len(w)
    assert w.min() == 0 and w.max() <= 12
    mean, var = w.mean(), w.var(ddof=1)
    print("mean", mean, "var", var)
    assert abs(mean - 1) <= 4 * math.sqrt(1.0 / N)                      # Poisson(1): variance 1
    assert abs(var - 1) <= 4 * math.sqrt(3.0 / N)                       # fourth central moment 4: var(s^2) ~ (4 - 1) / N
    # a weight depends on (seed, replicate, cluster) alone
    assert B.weights(0, 3, [5, 9, 5]).tolist()[0] == B.weights(0, 3, [5]).tolist()[0]
    assert B.weights(0, 3, np.arange(200)).tolist() != B.weights(1, 3, np.arange(200)).tolist()
    assert B.weights(0, 3, np.arange(200)).tolist() != B.weights(0, 4, np.arange(200)).tolist()


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for ea, eb in zip(ra, rb):
            assert ea == eb, (ea, eb)


def _case(name):
    rng = np.random.default_rng(5)
    if name == "random":
        n = 60
        return dict(y=rng.integers(0, 2, n), s=np.round(rng.random(n), 1).astype(np.float32), cluster=rng.integers(0, 15, n), n_rep=5)
    if name == "rows":
        n = 37
        return dict(y=rng.integers(0, 2, n), s=np.round(rng.random(n), 1).astype(np.float32), cluster=None, n_rep=4)
    if name == "tied":
        n = 40
        return dict(y=rng.integers(0, 2, n), s=np.full(n, 0.25, dtype=np.float32), cluster=rng.integers(0, 10, n), n_rep=4)
    if name == "zeros":
        return dict(y=[1, 0, 1, 0], s=np.array([0.0, -0.0, -0.0, 0.0], dtype=np.float32), cluster=[0, 1, 2, 3], n_rep=6)
    if name == "single":
        n = 20
        return dict(y=np.ones(n, dtype=np.int64), s=rng.random(n).astype(np.float32), cluster=rng.integers(0, 5, n), n_rep=3)
    if name == "domains":
        n = 90
        dom = rng.integers(0, 4, n)
        dom[dom == 2] = 3                                               # domain 2 is empty
        y = rng.integers(0, 2, n)
        y[dom == 1] = 0                                                 # domain 1 holds one class
        return dict(y=y, s=np.round(rng.random(n), 1).astype(np.float32), cluster=rng.integers(0, 12, n), n_rep=5, domain=dom,
                    n_domain=4, user_weight=rng.random(12) + 0.5)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["random", "rows", "tied", "zeros", "single", "domains"])
def test_brute_and_sorted_forms_agree_exactly(name):
    kw = _case(name)
    brute, fast = B.bootstrap_brute(seed=3, **kw), B.bootstrap_sorted(seed=3, **kw)
    _same(brute, fast)
    n_seg = kw.get("n_domain", 1) + 1
    assert len(brute) == kw["n_rep"] and all(len(r) == n_seg for r in brute)
    if name == "tied":
        assert all(e["auc"] in (None, Fraction(1, 2)) for r in brute for e in r) and any(e["auc"] for r in brute for e in r)
    if name == "zeros":                                                 # -0.0 ties +0.0
        assert all(e["auc"] in (None, Fraction(1, 2)) for r in brute for e in r)
    if name == "single":
        assert all(e["auc"] is None and e["loss"] is None and e["gauc"] is None for r in brute for e in r)
    if name == "domains":
        for r in brute:
            assert r[2]["W"] == 0 and r[2]["auc"] is None and r[1]["Wp"] == 0 and r[1]["auc"] is None
            assert r[4]["W"] == sum(e["W"] for e in r[:4]) and r[4]["Wp"] == sum(e["Wp"] for e in r[:4])   # shared weights
    if name == "rows":
        assert all(e["gauc"] is None for r in brute for e in r)         # no cluster column: no GAUC


def test_unit_weights_give_the_unweighted_helpers_figures():
    kw = _case("domains")
    y, s, u, dom, nd, uw = kw["y"], kw["s"], kw["cluster"], kw["domain"], kw["n_domain"], kw["user_weight"]
    for weights in (None, uw):
        got = B.bootstrap_sorted(y, s, u, 0, 1, dom, nd, weights, weight_fn=B.ones)[0]
        auc, loss, gauc = delong_exact(y, s, None, dom, nd), loss_ci_exact(y, s, None, dom, nd), gauc_ci_exact(y, s, u, dom, nd, weights)
        for d in range(nd + 1):
            assert got[d]["auc"] == auc[d]["auc"] and got[d]["W"] == auc[d]["rows"] and got[d]["Wp"] == auc[d]["P"]
            assert got[d]["loss"] == loss[d]["loss"]
            assert got[d]["gauc"] == gauc[d]["gauc"] and got[d]["K"] == gauc[d]["counted"]
    assert got[0]["auc"] is not None and got[0]["gauc"] is not None and got[2]["auc"] is None


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(a)
    return np.max(np.abs(a[ok] - b[ok]) / np.spacing(np.abs(b[ok]))) if ok.any() else 0.0


def test_summarize_bootstrap_agrees_with_numpy():
    from cdcmdr_amd.evaluate import summarize_bootstrap
    rng = np.random.default_rng(2)
    x = rng.random((57, 6)) * 0.2 + 0.6
    x[rng.random(x.shape) < 0.2] = np.nan
    x[:, 3] = np.nan                                                    # no valid replicate
    x[1:, 4] = np.nan                                                   # one valid replicate
    x[:, 5] = 0.5                                                       # no spread
    for level in (0.95, 0.8):
        se, lo, hi, valid = summarize_bootstrap(torch.from_numpy(x), level)
        cnt = (~np.isnan(x)).sum(0)
        assert valid.dtype == torch.int64 and valid.tolist() == cnt.tolist() and cnt[3] == 0 and cnt[4] == 1
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want_se = np.nanstd(x, axis=0, ddof=1)
                want_lo, want_hi = np.nanpercentile(x, [50 * (1 - level), 50 * (1 + level)], axis=0)
        for w in (want_se, want_lo, want_hi):
            w[cnt < 2] = np.nan
        assert se.dtype == torch.float64 and se.shape == (6,)
        assert _ulps(lo.numpy(), want_lo) <= 4 and _ulps(hi.numpy(), want_hi) <= 4
        assert se[5].item() == 0.0 and lo[5].item() == hi[5].item() == 0.5
        # the deviation's bound is relative to the spread it measures, not to a zero
        assert _ulps(se.numpy()[:3], want_se[:3]) <= 4
        assert np.isnan(se.numpy()[3:5]).all() and np.isnan(lo.numpy()[3:5]).all() and np.isnan(hi.numpy()[3:5]).all()
    # a replicate tensor with more axes keeps them
    se, lo, hi, valid = summarize_bootstrap(torch.from_numpy(x.reshape(57, 2, 3)))
    assert se.shape == lo.shape == hi.shape == valid.shape == (2, 3)
    with pytest.raises(ValueError):
        summarize_bootstrap(torch.from_numpy(x), 1.0)


def test_entry_point_refuses_bad_arguments_without_touching_the_device():
    from cdcmdr_amd import _lib
    lib = _lib.load()
    one, ws = C.c_void_p(16), C.c_void_p(256)
    big = 1 << 40

    def call(pred=one, pred_b=None, label=one, cluster=one, ld_c=1, n_c=10, domain=one, ld_d=1, n_domain=3, uw=None, n=100, n_rep=8,
             seed=0, gauc=1, out=one, counts=one, err=None, work=ws, nbytes=big):
        return lib.cdc_eval_bootstrap(pred, pred_b, label, cluster, ld_c, n_c, domain, ld_d, n_domain, uw, n, n_rep, seed, gauc, out,
                                      counts, err, work, nbytes, None)

    for bad in (dict(pred=None), dict(label=None), dict(out=None), dict(counts=None), dict(work=None)):
        assert call(**bad) < 0 and b"null pointer" in lib.cdc_last_error(), bad
    for bad in (dict(n=0), dict(n=-5), dict(n_domain=0), dict(n_domain=1 << 20), dict(ld_c=-1), dict(ld_d=-1), dict(n_c=0)):
        assert call(**bad) < 0 and b"bad sizes" in lib.cdc_last_error(), bad
    assert call(domain=None) < 0 and b"needs the domain column" in lib.cdc_last_error()
    for n_rep in (0, -1, 4097):
        assert call(n_rep=n_rep) < 0 and b"n_rep" in lib.cdc_last_error()
    assert call(cluster=None) < 0 and b"GAUC needs the cluster column" in lib.cdc_last_error()
    assert call(n=1 << 28) == -2 and b"2^28" in lib.cdc_last_error()
    assert call(n_c=1 << 31, n_domain=3) < 0 and b"group ids exceed 2^32" in lib.cdc_last_error()
    assert call(work=C.c_void_p(264)) < 0 and b"256-byte aligned" in lib.cdc_last_error()
    assert call(nbytes=1024) < 0 and b"workspace" in lib.cdc_last_error()
    assert call(cluster=None, gauc=0, nbytes=1024) < 0 and b"workspace" in lib.cdc_last_error()
    # the size query refuses the same sizes with 0 and never touches a device either
    q = lib.cdc_eval_bootstrap_workspace_bytes
    assert q(0, 3, 10, 8, 0) == 0 and q(1 << 28, 3, 10, 8, 0) == 0 and q(100, 0, 10, 8, 0) == 0
    assert q(100, 3, 10, 0, 0) == 0 and q(100, 3, 10, 4097, 0) == 0 and q(100, 3, 1 << 31, 8, 1) == 0 and q(100, 3, 0, 8, 1) == 0
    # the wrapper's own checks come before any device work as well
    from cdcmdr_amd.evaluate import eval_bootstrap
    p, y = torch.zeros(4), torch.zeros(4, dtype=torch.int16)
    with pytest.raises(ValueError, match="n_rep"):
        eval_bootstrap(p, y, n_rep=0)
    with pytest.raises(ValueError, match="gauc needs the cluster column"):
        eval_bootstrap(p, y, gauc=True)
    with pytest.raises(ValueError, match="n_cluster"):
        eval_bootstrap(p, y, cluster=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.HipExtensionError):
        eval_bootstrap(p, y)
