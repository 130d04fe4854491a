"""cdc_eval_calibration_bootstrap, eval_calibration_bootstrap and Evaluator(calibration_ci=True) on the device against
tests/calibration_boot_exact.py (pure-integer weights and exact rationals; tests/test_calibration_boot_cpu.py holds its two forms to
each other).  Nothing is left out of a comparison: every replicate, every segment, every figure.  u = 2^-53.

  w_rows, w_pos  equal to the helper's integers.
  NaN            exactly where the helper has None.
  the figures    tests/test_gpu_calibration.py's derived bound.  The kernel's sums are exact integers; every double is (an integer
                 numerator -> double: ONE rounding, also for the 96-bit sum of squares) / (W or Wp times a power of two: exact while
                 W < 2^53) — two roundings, (1 + u)^2 - 1; the expected value is the exact rational rounded once more (u / 2):
                     |device - exact| <= 4 u |exact|      (2.5 u are due).
                 The derivation needs W < 2^53 and numerators below 2^128: SQ <= W 2^32 and SE2 <= W 2^64, so W < 2^32 (12 rows'
                 weights times n < 2^28) keeps both — asserted on every segment.
Cross-checks between calls are device against device and bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import bootstrap_exact as B
import calibration_boot_exact as CB
from test_calibration_boot_cpu import brier_errors, clustered_case, rows_case
from test_gpu_bootstrap import _boundary_facts
from test_gpu_eval_ci import _columns, _f32, _tiny

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
FIELDS = ("pcoc", "brier", "ece", "ece_q")


def _tiles():
    from cdcmdr_amd.evaluate import CALBOOT_CHUNK, CALBOOT_REP_TILE
    return CALBOOT_CHUNK, CALBOOT_REP_TILE


def _device(cuda, y, p, K=10, cluster=None, n_cluster=None, seed=0, n_rep=1, dom=None, n_domain=1, pb=None, strided=False):
    """-> ({field: numpy [n_rep, n_domain + 1] or None}, err)"""
    from cdcmdr_amd.evaluate import eval_calibration_bootstrap
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    ct, dt = _columns(cuda, len(y), [cluster, dom], strided)
    r = eval_calibration_bootstrap(_f32(cuda, p), label, ct, n_cluster, dt, n_domain, K, n_rep, seed, pred_b=_f32(cuda, pb))
    assert r._fields == FIELDS + ("w_rows", "w_pos") + tuple(f + "_b" for f in FIELDS)
    for k, t in r._asdict().items():
        assert (t is None) == (k.endswith("_b") and pb is None), k
        if t is not None:
            assert t.is_cuda and tuple(t.shape) == (n_rep, n_domain + 1), (k, t.shape)
            assert t.dtype == (torch.int64 if k.startswith("w_") else torch.float64)
    err = int(eval_calibration_bootstrap.last_err.item())
    return {k: None if t is None else t.cpu().numpy().copy() for k, t in r._asdict().items()}, err


def _check(got, want, what="", suffix="", err=0):
    """every replicate, segment and figure of the device (fields with `suffix`) against the helper's [replicate][segment] dicts"""
    vals, got_err = got
    assert got_err == err, (what, got_err, err)
    n_rep, n_seg = vals["w_rows"].shape
    assert len(want) >= n_rep and len(want[0]) == n_seg
    for r in range(n_rep):
        for d in range(n_seg):
            w = want[r][d]
            assert w["W"] < 2 ** 32                              # the bound's derivation holds (module docstring)
            assert vals["w_rows"][r, d] == w["W"] and vals["w_pos"][r, d] == w["Wp"], (what, r, d, vals["w_rows"][r, d], w["W"])
            for k in FIELDS:
                g, e = vals[k + suffix][r, d], w[k]
                if e is None:
                    assert np.isnan(g), (what, k, r, d, g)
                else:
                    e = float(e)
                    assert abs(g - e) <= 4 * U * abs(e), (what, k, r, d, g, e, abs(g - e), 4 * U * abs(e))


def _bits(a, b, keys=None):
    for k in keys or a:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not np.array_equal(a[k].view(np.int64), b[k].view(np.int64)):
            return False
    return True


def _scores(rng, n):
    return (rng.integers(0, 11, n) / 10).astype(np.float32)                 # one decimal: ties everywhere


def _mass_cut_inside_tie(y, p, w, K):
    """a mass-bin boundary of the expanded rows falls between two copies of identical (score, label)"""
    order = np.lexsort((y, p))
    ke = np.repeat(np.asarray(p, dtype=np.float64)[order] * 4 + np.asarray(y)[order], w[order])
    W = len(ke)
    cuts = [(b * W) // K for b in range(1, K)]
    return any(0 < c < W and ke[c - 1] == ke[c] for c in cuts)


@pytest.mark.parametrize("per_cluster", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 5, 37])
def test_tiny_shapes_every_bin_count_and_replicate_tile(cuda, n, per_cluster):
    CH, RT = _tiles()
    rng = np.random.default_rng(100 + n)
    y, p = rng.integers(0, 2, n), _scores(rng, n)
    if n >= 2:
        y[:2], p[:2] = [1, 0], [-0.0, 0.0]                                  # a tied pair under the sign of zero
    if per_cluster == 1:
        cluster, n_cluster = rng.permutation(n), n
    else:
        n_cluster = max(1, n // 3)                                          # 3-4 rows per cluster
        cluster = rng.permutation(np.arange(n) % n_cluster)
    for K in (1, 2, 10, 1024):
        want = CB.direct(y, p, K, cluster, 11, RT + 1)
        for n_rep in (1, RT - 1, RT, RT + 1):
            _check(_device(cuda, y, p, K, cluster, n_cluster, 11, n_rep), want, f"tiny {n}/{per_cluster}/{K}/{n_rep}")
    if n == 37:                                                             # K = 1024 > W: empty bins, and a weight-3 row lies in three
        ws = [B.weights(11, r, cluster) for r in range(RT + 1)]
        assert all(0 < w.sum() < 1024 for w in ws) and max(int(w.max()) for w in ws) >= 3


def test_the_documented_example(cuda):
    # INTEGRATION.md's five rows of three users: dyadic predictions, every figure the correctly rounded quotient
    y, p, u = [1, 1, 0, 1, 0], [0.25, 1.0, 0.125, 0.75, 0.25], [0, 0, 1, 1, 2]
    assert [B.weights(0, r, np.arange(3)).tolist() for r in range(2)] == [[0, 2, 1], [2, 0, 0]]
    got, err = _device(cuda, y, p, 2, u, 3, 0, 2)
    assert err == 0 and got["w_rows"].tolist() == [[5, 5], [4, 4]] and got["w_pos"].tolist() == [[2, 2], [4, 4]]
    assert got["pcoc"][:, 1].tolist() == [1.0, 0.625] and got["brier"][:, 1].tolist() == [0.04375, 0.28125]
    assert got["ece"][:, 1].tolist() == [0.2, 0.375] and got["ece_q"][:, 1].tolist() == [0.1, 0.375]
    assert _device(cuda, y, p, 3, u, 3, 0, 2)[0]["ece_q"][:, 1].tolist() == [0.2, 0.375]     # a row's two copies in two bins


@pytest.mark.parametrize("n_domain", [1, 3])
@pytest.mark.parametrize("which", range(7))
def test_chunk_boundaries_tie_runs_and_segment_boundaries(cuda, which, n_domain):
    CH, RT = _tiles()
    n = [CH // 2 - 1, CH // 2, CH // 2 + 1, CH - 1, CH, CH + 1, 3 * CH // 2 + 17][which]       # the launch sorts 2 n keys
    rng = np.random.default_rng(200 + which)
    y, p = rng.integers(0, 2, n), _scores(rng, n)
    dom = None if n_domain == 1 else rng.integers(0, n_domain, n)
    n_cluster = n // 3
    cluster = rng.integers(0, n_cluster, n)
    straddle, inside = _boundary_facts(y, p, dom, n_domain, CH)
    assert inside or (n_domain == 1 and n % CH == 0)    # a segment starts inside a chunk (or, once, exactly on a chunk boundary)
    assert straddle == (2 * n > CH and n % CH != 0)     # a tie run lies across a chunk boundary (n = CH: the boundaries part segments)
    assert _mass_cut_inside_tie(y, p, B.weights(5, 0, cluster), 10)
    want = CB.by_expansion(y, p, 10, cluster, 5, RT + 1, dom, n_domain)
    _check(_device(cuda, y, p, 10, cluster, n_cluster, 5, RT + 1, dom, n_domain), want, f"chunk {n}/{n_domain}")


@pytest.mark.parametrize("K", [10, 15, 1024])
def test_many_workgroups_and_skewed_scores(cuda, K):
    CH, RT = _tiles()
    rng = np.random.default_rng(31)
    n = 5 * CH + 77
    p = (rng.random(n) ** 5).astype(np.float32)                             # most mass below 0.1: width bins of very unequal size
    p[rng.random(n) < 0.1] = np.float32(0.03125)                            # a tie run of ~500 rows
    p[:3] = [0.0, 1.0, 0.5]
    y = (rng.random(n) < 0.03 + 0.6 * p).astype(np.int16)
    dom, cluster = rng.integers(0, 3, n), rng.integers(0, 700, n)
    want = CB.by_expansion(y, p, K, cluster, 3, 3, dom, 3)
    _check(_device(cuda, y, p, K, cluster, 700, 3, 3, dom, 3), want, f"many/{K}")


def test_segments_empty_single_class_and_a_segment_of_weight_zero(cuda):
    CH, RT = _tiles()
    rng = np.random.default_rng(3)
    n, n_rep = 300, 2 * RT + 3
    dom = rng.integers(0, 5, n)
    dom[dom == 1] = 0                                                       # domain 1: empty
    y, p = rng.integers(0, 2, n), _scores(rng, n)
    y[dom == 2] = 1                                                         # domain 2: one class
    y[dom == 4] = 0                                                         # domain 4: the other one
    two = np.flatnonzero(dom == 3)
    dom[two[2:]] = 0                                                        # domain 3: two rows of ONE cluster
    cluster = rng.integers(0, 60, n)
    cluster[two[:2]] = 60
    want = CB.direct(y, p, 10, cluster, 21, n_rep, dom, 5)
    got = _device(cuda, y, p, 10, cluster, 61, 21, n_rep, dom, 5)
    _check(got, want, "segments")
    assert all(r[1]["W"] == 0 and r[1]["brier"] is None for r in want)
    assert all(r[2]["pcoc"] is not None and r[2]["brier"] is not None and r[2]["ece"] is not None for r in want)   # a single class
    assert all(r[4]["W"] > 0 and r[4]["pcoc"] is None and r[4]["brier"] is not None and r[4]["ece_q"] is not None for r in want)
    dead = [r[3]["W"] == 0 for r in want]                                   # seed 21 gives the cluster weight 0 in some replicates
    assert any(dead) and not all(dead)
    for k in FIELDS:
        assert np.isnan(got[0][k][:, 3]).tolist() == dead, k
        assert np.isnan(got[0][k][:, 1]).all()
    assert np.isnan(got[0]["pcoc"][:, 4]).all() and not np.isnan(got[0]["brier"][:, 4]).any()
    # fifty domains over 400 rows: many segments inside one chunk, most mass bins empty at K = 64
    n = 400
    dom, y, p, cluster = rng.integers(0, 50, n), rng.integers(0, 2, n), _scores(rng, n), rng.integers(0, 40, n)
    _check(_device(cuda, y, p, 64, cluster, 40, 2, RT + 1, dom, 50), CB.direct(y, p, 64, cluster, 2, RT + 1, dom, 50), "fifty")


@functools.lru_cache(maxsize=None)
def _shared():
    """one input of clusters that span domains, and its references: shared by the tests below and left unchanged"""
    CH, RT = _tiles()
    rng = np.random.default_rng(4)
    n, n_cluster, n_rep = 240, 30, RT + 2
    y, p, dom, cluster = rng.integers(0, 2, n), _scores(rng, n), rng.integers(0, 3, n), rng.integers(0, n_cluster, n)
    pb = p.copy()
    flip = rng.choice(n, 9, replace=False)
    pb[flip] = np.float32(1.0) - pb[flip]                                   # a second vector that differs in a few rows
    want = CB.direct(y, p, 7, cluster, 77, n_rep, dom, 3)
    want_b = CB.direct(y, pb, 7, cluster, 77, n_rep, dom, 3)
    want_rows = CB.direct(y, p, 7, None, 77, n_rep, dom, 3)
    return n, n_cluster, n_rep, y, p, pb, dom, cluster, want, want_b, want_rows


@pytest.mark.parametrize("strided", [False, True])
def test_clusters_span_domains_and_counts_equal_eval_bootstrap(cuda, strided):
    from cdcmdr_amd.evaluate import eval_bootstrap
    n, n_cluster, n_rep, y, p, pb, dom, cluster, want, want_b, want_rows = _shared()
    got = _device(cuda, y, p, 7, cluster, n_cluster, 77, n_rep, dom, 3, strided=strided)
    _check(got, want, f"span/{strided}")
    label = torch.from_numpy(y.astype(np.int16)).to(cuda)
    ct, dt = _columns(cuda, n, [cluster, dom], strided)
    boot = eval_bootstrap(_f32(cuda, p), label, ct, n_cluster, dt, 3, n_rep, 77)
    assert np.array_equal(boot.w_rows.cpu().numpy(), got[0]["w_rows"]) and np.array_equal(boot.w_pos.cpu().numpy(), got[0]["w_pos"])
    # rows as their own clusters
    rows = _device(cuda, y, p, 7, None, None, 77, n_rep, dom, 3, strided=strided)
    _check(rows, want_rows, f"rows/{strided}")
    boot = eval_bootstrap(_f32(cuda, p), label, None, None, dt, 3, n_rep, 77)
    assert np.array_equal(boot.w_rows.cpu().numpy(), rows[0]["w_rows"]) and np.array_equal(boot.w_pos.cpu().numpy(), rows[0]["w_pos"])
    same = _device(cuda, y, p, 7, np.arange(n), n, 77, n_rep, dom, 3, strided=strided)
    assert _bits(rows[0], same[0])


def test_paired_vectors_share_the_weights(cuda):
    n, n_cluster, n_rep, y, p, pb, dom, cluster, want, want_b, want_rows = _shared()
    got = _device(cuda, y, p, 7, cluster, n_cluster, 77, n_rep, dom, 3, pb=pb)
    _check(got, want, "paired a")
    _check(got, want_b, "paired b", suffix="_b")
    alone_a = _device(cuda, y, p, 7, cluster, n_cluster, 77, n_rep, dom, 3)[0]
    alone_b = _device(cuda, y, pb, 7, cluster, n_cluster, 77, n_rep, dom, 3)[0]
    assert _bits(got[0], alone_a, FIELDS + ("w_rows", "w_pos"))
    assert _bits({k: got[0][k + "_b"] for k in FIELDS}, alone_b, FIELDS)     # the second unpaired call, bit for bit
    assert not _bits(got[0], {"brier": got[0]["brier_b"]}, ("brier",))
    same = _device(cuda, y, p, 7, cluster, n_cluster, 77, n_rep, dom, 3, pb=p.copy())[0]
    for k in FIELDS:
        assert _bits(same, {k: same[k + "_b"]}, (k,)), k                    # identical bits:
        d = same[k] - same[k + "_b"]
        assert np.all((d == 0) | np.isnan(same[k]))                         # every delta is 0


def test_row_order_and_seed(cuda):
    n, n_cluster, n_rep, y, p, pb, dom, cluster, want, want_b, want_rows = _shared()
    got = _device(cuda, y, p, 7, cluster, n_cluster, 77, n_rep, dom, 3, pb=pb)
    perm = np.random.default_rng(1).permutation(n)
    moved = _device(cuda, y[perm], p[perm], 7, cluster[perm], n_cluster, 77, n_rep, dom[perm], 3, pb=pb[perm])
    assert _bits(got[0], moved[0])                                          # every output, both vectors
    other = _device(cuda, y, p, 7, cluster, n_cluster, 78, n_rep, dom, 3, pb=pb)
    assert not _bits(got[0], other[0], ("w_rows",)) and not _bits(got[0], other[0], ("brier",))


def test_a_replicate_is_eval_calibration_on_the_repeated_rows(cuda):
    from cdcmdr_amd.evaluate import eval_calibration
    CH, RT = _tiles()
    rng = np.random.default_rng(41)
    n = CH + 300                                                            # three chunks of sorted positions
    y, p, dom, cluster = rng.integers(0, 2, n), _scores(rng, n), rng.integers(0, 3, n), rng.integers(0, 200, n)
    p[::7] = rng.random(len(p[::7])).astype(np.float32)
    n_rep = RT + 3
    got = _device(cuda, y, p, 10, cluster, 200, 9, n_rep, dom, 3)[0]
    pt, yt, dt = _f32(cuda, p), torch.from_numpy(y.astype(np.int16)).to(cuda), torch.from_numpy(dom.astype(np.int32)).to(cuda)
    for r in (0, 1, RT - 1, RT, n_rep - 1):
        w = torch.from_numpy(B.weights(9, r, cluster)).to(cuda)
        cal = eval_calibration(torch.repeat_interleave(pt, w), torch.repeat_interleave(yt, w), torch.repeat_interleave(dt, w), 3, 10)
        assert np.array_equal(cal.rows.cpu().numpy(), got["w_rows"][r]) and np.array_equal(cal.positives.cpu().numpy(), got["w_pos"][r])
        for k in FIELDS:
            mine, theirs = got[k][r], getattr(cal, k).cpu().numpy()
            assert not np.isnan(theirs).any()
            assert np.array_equal(mine.view(np.int64), theirs.view(np.int64)), (r, k, mine, theirs)


def test_bad_rows_set_the_error_word_and_are_counted_clamped(cuda):
    y = np.array([0, 1, 1, 0, 1, 0])
    p = np.array([0.2, 0.3, 0.7, 0.6, 0.1, 0.9], dtype=np.float32)
    dom, cl = np.array([0, 1, 0, 1, 1, 0]), np.array([0, 0, 1, 1, 2, 2])
    assert _device(cuda, y, p, 4, cl, 3, 1, 3, dom, 2)[1] == 0
    bad_p = p.copy()
    bad_p[[1, 3, 4]] = [1.5, np.nan, -0.25]                                 # counted as 1, 0, 0; row 4 is the largest
    _check(_device(cuda, y, bad_p, 4, cl, 3, 1, 3, dom, 2), CB.direct(y, CB.clip01(bad_p), 4, cl, 1, 3, dom, 2), "pred", err=5)
    bad_d = dom.copy()
    bad_d[[0, 2]] = [-3, 2]                                                 # counted in domains 0 and 1
    _check(_device(cuda, y, p, 4, cl, 3, 1, 3, bad_d, 2), CB.direct(y, p, 4, cl, 1, 3, np.clip(bad_d, 0, 1), 2), "domain", err=3)
    bad_c = cl.copy()
    bad_c[[3, 5]] = [-1, 3]                                                 # counted as clusters 0 and 2
    _check(_device(cuda, y, p, 4, bad_c, 3, 1, 3, dom, 2), CB.direct(y, p, 4, np.clip(bad_c, 0, 2), 1, 3, dom, 2), "cluster", err=6)
    bad_y = y.copy()
    bad_y[2] = 2                                                            # counted as a positive
    _check(_device(cuda, bad_y, p, 4, cl, 3, 1, 3, dom, 2), CB.direct(y, p, 4, cl, 1, 3, dom, 2), "label", err=3)
    assert _device(cuda, y, p, 4, cl, 3, 1, 3, dom, 2, pb=bad_p)[1] == 5    # a bad prediction in pred_b alone


def test_brier_replicates_spread_like_the_analytic_errors_on_the_device(cuda):
    """tests/test_calibration_boot_cpu.py's two cases and assertions on the device's replicates (400 of them, seed 7)"""
    from cdcmdr_amd.evaluate import eval_calibration_bootstrap, summarize_bootstrap
    p, y = rows_case()
    r = eval_calibration_bootstrap(_f32(cuda, p), torch.from_numpy(y).to(cuda), n_rep=400, seed=7)
    se, lo, hi, valid = summarize_bootstrap(r.brier)
    assert se.is_cuda and valid.tolist() == [400, 400]
    ratio_rows = se[1].item() / brier_errors(p, y)[0]
    pc, yc, user = clustered_case()
    r = eval_calibration_bootstrap(_f32(cuda, pc), torch.from_numpy(yc).to(cuda), torch.from_numpy(user).to(cuda), 400, n_rep=400, seed=7)
    spread = summarize_bootstrap(r.brier)[0][1].item()
    rows_c, clustered_se = brier_errors(pc, yc, user)
    print("rows case: ratio", ratio_rows, "clustered case: against clustered", spread / clustered_se, "against rows", spread / rows_c)
    assert abs(ratio_rows - 1) <= 0.15
    assert abs(spread / clustered_se - 1) <= 0.15
    assert spread >= 1.2 * rows_c


def _downsampled(cuda):
    """tests/test_gpu_eval_ci.py's tiny model and rows with labels drawn from the model's own predictions shifted by +1.2 on the logit
    scale: what a model trained before the negatives were down-sampled looks like on the down-sampled set"""
    from cdcmdr_amd.evaluate import Evaluator
    model, loader, X, _ = _tiny(cuda)
    p = Evaluator(model, mode="multi").predict(loader)[0].cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(17)
    y = (rng.random(len(p)) < 1.0 / (1.0 + np.exp(-(np.log(p / (1 - p)) + 1.2)))).astype(np.int16)
    out, i = [], 0
    for Xb, _, gb in loader:
        out.append((Xb, torch.from_numpy(y[i:i + len(Xb)]).to(cuda).reshape(-1, 1), gb))
        i += len(Xb)
    return model, out, X, y


def test_evaluator_calibration_ci(cuda):
    from cdcmdr_amd.evaluate import Evaluator, _z, eval_calibration, eval_calibration_bootstrap, summarize_bootstrap
    model, loader, X, y = _downsampled(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    kw = dict(mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w, user_idx=2, n_user=40, calibration=5, bootstrap=40,
              bootstrap_seed=5, bootstrap_level=0.9)
    for missing in ("calibration", "bootstrap"):
        with pytest.raises(ValueError, match="calibration_ci needs calibration"):
            Evaluator(model, calibration_ci=True, **{k: v for k, v in kw.items() if k != missing})
    # off: exactly the keys and values of an evaluator built without the keyword
    plain, off = Evaluator(model, **kw), Evaluator(model, calibration_ci=False, **kw)
    res0 = plain.test(loader)
    assert off.test(loader) == res0 and not any("pcoc_boot" in k or "ece_boot" in k for k in res0)
    cmp0 = plain.compare(plain, loader)
    cmp_off = off.compare(off, loader)
    assert sorted(cmp0) == sorted(cmp_off) and not any("ece" in k or "brier" in k or "pcoc" in k for k in cmp0)
    for k in cmp0:
        a, b = cmp0[k], cmp_off[k]
        assert a == b or (a != a and b != b) or (isinstance(a, dict) and all(a[d] == b[d] or a[d] != a[d] for d in a)), k
    # on: test()
    ev = Evaluator(model, calibration_ci=True, **kw)
    res = ev.test(loader)
    figs = ("pcoc", "brier", "ece", "ece_quantile")
    new = [f"{scope}_{f}_boot_{what}" for scope in ("total", "domain", "mean") for f in figs for what in ("se", "lo", "hi")]
    assert sorted(res) == sorted(list(res0) + new)
    for k in res0:
        if k != "boot_valid":
            assert res[k] == res0[k], k                        # the other figures are untouched
    pred, label, dom, user = ev._score(loader)
    cb = eval_calibration_bootstrap(pred, label, user, 40, dom, 3, 5, 40, 5)
    wv = torch.tensor([w[d] for d in range(3)], dtype=torch.float64, device=cuda)
    valid = [res0["boot_valid"]]
    for f, reps in zip(figs, (cb.pcoc, cb.brier, cb.ece, cb.ece_q)):
        mean = (reps[:, :3] * wv).sum(1)                        # formed per replicate
        se, lo, hi, ok = (t.cpu().tolist() for t in summarize_bootstrap(torch.cat([reps, mean[:, None]], 1), 0.9))
        valid += ok
        for what, v in (("se", se), ("lo", lo), ("hi", hi)):
            assert res[f"total_{f}_boot_{what}"] == v[3] and res[f"mean_{f}_boot_{what}"] == v[4], (f, what)
            assert res[f"domain_{f}_boot_{what}"] == {d: v[d] for d in range(3)}
        assert res[f"total_{f}_boot_se"] > 0 and res[f"total_{f}_boot_lo"] < res["total_" + f] < res[f"total_{f}_boot_hi"]
    assert res["boot_valid"] == min(valid) == 40
    # compare() of a model against itself: deltas 0, z NaN
    self_cmp = ev.compare(ev, loader)
    delta_keys = [f"{scope}_{f}_{what}" for scope in ("total", "domain", "mean") for f in figs
                  for what in ("delta", "z", "delta_boot_se", "delta_boot_lo", "delta_boot_hi")]
    assert sorted(self_cmp) == sorted(list(cmp0) + delta_keys)
    for f in figs:
        assert self_cmp[f"total_{f}_delta"] == 0.0 and self_cmp[f"mean_{f}_delta"] == 0.0 and self_cmp[f"total_{f}_delta_boot_se"] == 0.0
        assert math.isnan(self_cmp[f"total_{f}_z"]) and math.isnan(self_cmp[f"mean_{f}_z"])
        assert all(v == 0.0 for v in self_cmp[f"domain_{f}_delta"].values()) and all(math.isnan(v) for v in self_cmp[f"domain_{f}_z"].values())
    # the recalibrated model against the raw one: ECE drops, and the interval of the drop excludes 0
    recal = plain.fit_recalibration(loader, method="bias")
    fixed = Evaluator(model, calibration_ci=True, recalibration=recal, **kw)
    both = fixed.compare(ev, loader)
    pr = fixed.predict(loader)[0]
    ca, cr = eval_calibration(pr, label, dom, 3, 5), eval_calibration(pred, label, dom, 3, 5)
    pair = eval_calibration_bootstrap(pr, label, user, 40, dom, 3, 5, 40, 5, pred_b=pred)
    for f, a, b, ra, rb in (("pcoc", ca.pcoc, cr.pcoc, pair.pcoc, pair.pcoc_b), ("brier", ca.brier, cr.brier, pair.brier, pair.brier_b),
                            ("ece", ca.ece, cr.ece, pair.ece, pair.ece_b), ("ece_quantile", ca.ece_q, cr.ece_q, pair.ece_q, pair.ece_q_b)):
        delta = (a - b).cpu().tolist()
        reps = ra - rb
        se, lo, hi, _ = (t.cpu().tolist() for t in summarize_bootstrap(torch.cat([reps, (reps[:, :3] * wv).sum(1)[:, None]], 1), 0.9))
        assert both[f"total_{f}_delta"] == delta[3] and both[f"domain_{f}_delta"] == {d: delta[d] for d in range(3)}
        assert both[f"mean_{f}_delta"] == sum(w[d] * delta[d] for d in range(3))
        assert (both[f"total_{f}_delta_boot_se"], both[f"total_{f}_delta_boot_lo"], both[f"total_{f}_delta_boot_hi"]) == (se[3], lo[3], hi[3])
        assert both[f"mean_{f}_delta_boot_se"] == se[4] and both[f"domain_{f}_delta_boot_hi"] == {d: hi[d] for d in range(3)}
        assert both[f"total_{f}_z"] == _z(delta[3], se[3]) and both[f"domain_{f}_z"] == {d: _z(delta[d], se[d]) for d in range(3)}
        assert both[f"mean_{f}_z"] == _z(both[f"mean_{f}_delta"], se[4])
    print("total_ece_delta", both["total_ece_delta"], "interval", both["total_ece_delta_boot_lo"], both["total_ece_delta_boot_hi"])
    assert both["total_ece_delta"] < 0 and both["total_ece_delta_boot_hi"] < 0 and both["total_ece_z"] < -2
    # the helper alone shows the same on these predictions, with margin: the drop is several times the interval's width away from 0
    pa, pb = pr.cpu().numpy(), pred.cpu().numpy()
    users, doms = X[:, 2], X[:, 3]
    ha, hb = (CB.as_array(CB.by_expansion(y, v, 5, users, 5, 40, doms, 3), "ece")[:, 3] for v in (pa, pb))
    h_lo, h_hi = np.percentile(ha - hb, [5, 95])
    print("helper interval", h_lo, h_hi)
    assert h_hi < -0.05 and h_hi < -2 * (h_hi - h_lo)
    assert abs(both["total_ece_delta_boot_hi"] - h_hi) <= 1e-12 and abs(both["total_ece_delta_boot_lo"] - h_lo) <= 1e-12
    # the user column is the cluster column: the other evaluator must see it too
    with pytest.raises(ValueError, match="different user columns"):
        ev.compare(Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w), loader)
