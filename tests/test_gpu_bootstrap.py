"""cdc_eval_bootstrap, eval_bootstrap / summarize_bootstrap and Evaluator(bootstrap=R) on the device against tests/bootstrap_exact.py
(pure-integer weights, exact rationals, math.log and math.fsum; tests/test_bootstrap_cpu.py holds its two forms to each other).
Nothing is left out of a comparison: every replicate, every segment, every figure.  u = 2^-53.

  w_rows, w_pos  equal to the helper's integers.
  NaN            exactly where the helper has None.
  auc            the device forms U2 and 2 Wp Wn as 64-bit integers and divides once.  Every shape here has 2 Wp Wn < 2^53 (asserted), so
                 both convert exactly and the quotient is the correctly rounded one: the bits of float(Fraction).
  loss           want = fsum(w_i l_i) / W over the segment's m rows.  The device's l_i differs from the helper's by two logarithms of
                 1 ulp each, this project's convention in tests/test_gpu_eval_ci.py: 2^-51 l_i, hence 2^-51 want on the sum of the
                 non-negative terms.  On top of that the device adds at most m terms >= 0 in some order (m u of the sum), converts W
                 (exact below 2^53) and divides (u); the helper's fsum and its division round once each (2 u):
                     |got - want| <= (2^-51 + (m + 3) u) want.
  gauc           tests/test_gpu_gauc.py's bound for sum w A / sum w over K counted groups is (2 K + 8) u |G|; here the weight of a
                 group is the product of the replicate's integer and omega_g, one more rounding in the numerator and one in the
                 denominator:
                     |got - want| <= (2 K + 10) u |G|.
"""
import functools

import numpy as np
import pytest
import torch

import bootstrap_exact as B
from test_gpu_eval_ci import _columns, _f32, _tiny

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _tiles():
    from cdcmdr_amd.evaluate import BOOT_CHUNK, BOOT_REP_TILE
    return BOOT_CHUNK, BOOT_REP_TILE


def _device(cuda, y, s, cluster=None, n_cluster=None, seed=0, n_rep=1, dom=None, n_domain=1, uw=None, gauc=None, sb=None, strided=False):
    """-> ({field: numpy [n_rep, n_domain + 1] or None}, err)"""
    from cdcmdr_amd.evaluate import eval_bootstrap
    label = torch.from_numpy(np.array(y).astype(np.int16)).to(cuda)
    ct, dt = _columns(cuda, len(y), [cluster, dom], strided)
    wt = None if uw is None else torch.from_numpy(np.asarray(uw, dtype=np.float64)).to(cuda)
    r = eval_bootstrap(_f32(cuda, s), label, ct, n_cluster, dt, n_domain, n_rep, seed, wt, gauc, pred_b=_f32(cuda, sb))
    assert r._fields == ("auc", "loss", "gauc", "w_rows", "w_pos", "auc_b", "loss_b", "gauc_b")
    want_gauc = (cluster is not None) if gauc is None else gauc
    for k, t in r._asdict().items():
        absent = (k.startswith("gauc") and not want_gauc) or (k.endswith("_b") and sb is None)
        assert (t is None) == absent, k
        if t is not None:
            assert t.is_cuda and tuple(t.shape) == (n_rep, n_domain + 1), (k, t.shape)
            assert t.dtype == (torch.int64 if k.startswith("w_") else torch.float64)
    err = int(eval_bootstrap.last_err.item())
    return {k: None if t is None else t.cpu().numpy().copy() for k, t in r._asdict().items()}, err


def _check(got, want, what="", suffix="", err=0):
    """every replicate and segment of the device's figures (fields with `suffix`) against the helper's [replicate][segment] dicts"""
    vals, got_err = got
    assert got_err == err, (what, got_err, err)
    n_rep, n_seg = vals["w_rows"].shape
    assert len(want) >= n_rep and len(want[0]) == n_seg
    for r in range(n_rep):
        for d in range(n_seg):
            w = want[r][d]
            assert vals["w_rows"][r, d] == w["W"] and vals["w_pos"][r, d] == w["Wp"], (what, r, d, vals["w_rows"][r, d], w["W"])
            auc, loss = vals["auc" + suffix][r, d], vals["loss" + suffix][r, d]
            if w["auc"] is None:
                assert np.isnan(auc) and np.isnan(loss), (what, r, d, auc, loss)
            else:
                assert 2 * w["Wp"] * (w["W"] - w["Wp"]) < 2 ** 53
                assert auc == float(w["auc"]), (what, "auc", r, d, auc, float(w["auc"]))
                bound = (2.0 ** -51 + (w["rows"] + 3) * U) * w["loss"]
                assert abs(loss - w["loss"]) <= bound, (what, "loss", r, d, loss, w["loss"], abs(loss - w["loss"]), bound)
            if vals["gauc" + suffix] is None:
                continue
            g = vals["gauc" + suffix][r, d]
            if w["gauc"] is None:
                assert np.isnan(g), (what, "gauc", r, d, g)
            else:
                G = float(w["gauc"])
                bound = (2 * w["K"] + 10) * U * abs(G)
                assert abs(g - G) <= bound, (what, "gauc", r, d, g, G, abs(g - G), bound)


def _bits(a, b, keys=None):
    for k in keys or a:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not np.array_equal(a[k].view(np.int64), b[k].view(np.int64)):
            return False
    return True


def _scores(rng, n):
    return (rng.integers(0, 11, n) / 10).astype(np.float32)                 # one decimal: ties everywhere


@pytest.mark.parametrize("per_cluster", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 5, 37])
def test_tiny_against_the_pair_count(cuda, n, per_cluster):
    CH, RT = _tiles()
    rng = np.random.default_rng(100 + n)
    y, s = rng.integers(0, 2, n), _scores(rng, n)
    if n >= 2:
        y[:2], s[:2] = [1, 0], [-0.0, 0.0]                                  # a tied pair under the sign of zero
    if per_cluster == 1:
        cluster, n_cluster = rng.permutation(n), n
    else:
        n_cluster = max(1, n // 3)                                          # 3-4 rows per cluster
        cluster = rng.permutation(np.arange(n) % n_cluster)
    want = B.bootstrap_brute(y, s, cluster, 11, RT + 1)
    for n_rep in (1, RT - 1, RT, RT + 1):
        _check(_device(cuda, y, s, cluster, n_cluster, 11, n_rep), want, f"tiny {n}/{per_cluster}/{n_rep}")
    if n == 37:
        assert sum(e["auc"] is not None for r in want for e in r) == 2 * (RT + 1)


def _layout(y, s, dom, n_domain):
    """the device's sorted order of (segment, score) -> (segment of every sorted position, score of every sorted position)"""
    y, s = np.asarray(y), np.asarray(s, dtype=np.float32) + np.float32(0.0)
    d = np.zeros(len(y), dtype=np.int64) if dom is None else np.asarray(dom)
    seg, sc = np.r_[d, np.full(len(y), n_domain)], np.r_[s, s]
    order = np.lexsort((sc, seg))
    return seg[order], sc[order]


def _boundary_facts(y, s, dom, n_domain, CH):
    """(a tie run straddles a chunk boundary, a segment boundary lies strictly inside a chunk)"""
    seg, sc = _layout(y, s, dom, n_domain)
    cuts = np.arange(CH, len(seg), CH)
    straddle = bool(np.any((seg[cuts] == seg[cuts - 1]) & (sc[cuts] == sc[cuts - 1]))) if len(cuts) else False
    starts = np.flatnonzero(seg[1:] != seg[:-1]) + 1
    inside = bool(np.any(starts % CH != 0))
    return straddle, inside


@pytest.mark.parametrize("n_domain", [1, 3])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_chunk_boundaries_against_the_sorted_form(cuda, which, n_domain):
    CH, RT = _tiles()
    n = [CH // 2 - 1, CH // 2, CH // 2 + 1, 3 * CH // 2 + 17][which]        # the launch sorts 2 n keys
    rng = np.random.default_rng(200 + which)
    y, s = rng.integers(0, 2, n), _scores(rng, n)
    dom = None if n_domain == 1 else rng.integers(0, n_domain, n)
    n_cluster = n // 3
    cluster = rng.integers(0, n_cluster, n)
    straddle, inside = _boundary_facts(y, s, dom, n_domain, CH)
    assert inside and straddle == (2 * n > CH)                              # whenever there is a chunk boundary a tie run lies across it
    want = B.bootstrap_sorted(y, s, cluster, 5, RT + 1, dom, n_domain)
    _check(_device(cuda, y, s, cluster, n_cluster, 5, RT + 1, dom, n_domain), want, f"chunk {n}/{n_domain}")


@pytest.mark.parametrize("n_domain", [1, 3])
def test_all_scores_equal_is_one_half_across_chunks(cuda, n_domain):
    CH, RT = _tiles()
    n = 3 * CH // 2 + 17                                                    # "all rows" is one tie run over three chunks
    rng = np.random.default_rng(7)
    y, s = rng.integers(0, 2, n), np.full(n, 0.3, dtype=np.float32)
    dom = None if n_domain == 1 else rng.integers(0, n_domain, n)
    cluster = rng.integers(0, 300, n)
    got = _device(cuda, y, s, cluster, 300, 9, RT, dom, n_domain)
    assert np.all(got[0]["auc"] == 0.5) and np.all(got[0]["gauc"] == 0.5)
    _check(got, B.bootstrap_sorted(y, s, cluster, 9, RT, dom, n_domain), f"tied/{n_domain}")


def test_segments_empty_single_class_two_rows_and_fifty_domains(cuda):
    CH, RT = _tiles()
    rng = np.random.default_rng(3)
    n, n_rep = 300, 2 * RT + 3
    dom = rng.integers(0, 5, n)
    dom[dom == 1] = 0                                                       # domain 1: empty
    y, s = rng.integers(0, 2, n), _scores(rng, n)
    y[dom == 2] = 1                                                         # domain 2: one class
    two = np.flatnonzero(dom == 3)
    dom[two[2:]] = 4                                                        # domain 3: two rows, one of each class, two clusters
    y[two[:2]] = [1, 0]
    cluster = rng.integers(0, 60, n)
    cluster[two[:2]] = [60, 61]
    want = B.bootstrap_sorted(y, s, cluster, 21, n_rep, dom, 5)
    got = _device(cuda, y, s, cluster, 62, 21, n_rep, dom, 5)
    _check(got, want, "segments")
    assert all(r[1]["W"] == 0 and r[1]["auc"] is None and r[2]["auc"] is None and r[2]["gauc"] is None for r in want)
    live = [r[3]["auc"] is not None for r in want]
    assert any(live) and not all(live)                                      # a replicate that loses a class is NaN, the others are not
    assert np.isnan(got[0]["auc"][:, 3]).tolist() == [not v for v in live]
    assert np.isnan(got[0]["auc"][:, 1:3]).all() and np.isnan(got[0]["loss"][:, 1:3]).all()
    # fifty domains over 400 rows: many segments inside one chunk
    n = 400
    dom, y, s, cluster = rng.integers(0, 50, n), rng.integers(0, 2, n), _scores(rng, n), rng.integers(0, 40, n)
    _check(_device(cuda, y, s, cluster, 40, 2, RT + 1, dom, 50), B.bootstrap_sorted(y, s, cluster, 2, RT + 1, dom, 50), "fifty")


@functools.lru_cache(maxsize=None)
def _shared():
    """one input of clusters that span domains, and its reference: shared by the tests below and left unchanged"""
    CH, RT = _tiles()
    rng = np.random.default_rng(4)
    n, n_cluster, n_rep = 240, 30, RT + 2
    y, s, dom, cluster = rng.integers(0, 2, n), _scores(rng, n), rng.integers(0, 3, n), rng.integers(0, n_cluster, n)
    sb = s.copy()
    flip = rng.choice(n, 9, replace=False)
    sb[flip] = np.float32(1.0) - sb[flip]                                   # a second vector that differs in a few rows
    uw = rng.random(n_cluster) + 0.5
    want = {w is not None: B.bootstrap_sorted(y, s, cluster, 77, n_rep, dom, 3, w) for w in (None, uw)}
    want_b = B.bootstrap_sorted(y, sb, cluster, 77, n_rep, dom, 3)
    want_rows = B.bootstrap_sorted(y, s, None, 77, n_rep, dom, 3)
    return n, n_cluster, n_rep, y, s, sb, dom, cluster, uw, want, want_b, want_rows


@pytest.mark.parametrize("strided", [False, True])
def test_clusters_span_domains_and_share_their_weights(cuda, strided):
    n, n_cluster, n_rep, y, s, sb, dom, cluster, uw, want, want_b, want_rows = _shared()
    assert sum(len(set(dom[cluster == c])) > 1 for c in range(n_cluster)) > n_cluster // 2     # clusters do span domains
    got = _device(cuda, y, s, cluster, n_cluster, 77, n_rep, dom, 3, strided=strided)
    _check(got, want[False], f"span/{strided}")
    v = got[0]
    assert np.array_equal(v["w_rows"][:, 3], v["w_rows"][:, :3].sum(1)) and np.array_equal(v["w_pos"][:, 3], v["w_pos"][:, :3].sum(1))
    for r in range(n_rep):                                                  # the "all" column and the domain columns of ONE replicate
        w = B.weights(77, r, cluster)                                       # carry one weight vector
        assert [int(w[dom == d].sum()) for d in range(3)] + [int(w.sum())] == v["w_rows"][r].tolist()
    _check(_device(cuda, y, s, cluster, n_cluster, 77, n_rep, dom, 3, uw=uw, strided=strided), want[True], f"user_weight/{strided}")


def test_row_bootstrap_without_a_cluster_column(cuda):
    n, n_cluster, n_rep, y, s, sb, dom, cluster, uw, want, want_b, want_rows = _shared()
    got = _device(cuda, y, s, None, None, 77, n_rep, dom, 3)
    assert got[0]["gauc"] is None
    _check(got, want_rows, "rows")
    # the row index as an explicit cluster column: the same replicates, now with a GAUC of one-row users (none has both classes)
    same = _device(cuda, y, s, np.arange(n), n, 77, n_rep, dom, 3)
    assert _bits(got[0], same[0], ("auc", "loss", "w_rows", "w_pos")) and np.isnan(same[0]["gauc"]).all()


def test_a_cluster_out_of_range_sets_the_error_word(cuda):
    y, s = [0, 1, 1, 0, 1], np.array([0.2, 0.3, 0.7, 0.6, 0.1], dtype=np.float32)
    assert _device(cuda, y, s, [0, 0, 1, 1, 2], 3, 1, 3)[1] == 0
    got = _device(cuda, y, s, [0, 0, 1, 3, 2], 3, 1, 3)                     # cluster == n_cluster: counted as cluster 2
    _check(got, B.bootstrap_brute(y, s, [0, 0, 1, 2, 2], 1, 3), "clamped", err=4)
    assert _device(cuda, y, s, [0, 0, -1, 1, 2], 3, 1, 3, sb=s)[1] == 3
    bad = s.copy()
    bad[1] = np.nan
    assert _device(cuda, y, s, None, None, 1, 3, sb=bad)[1] == 2            # a NaN in pred_b alone
    assert _device(cuda, [0, 1, 2, 0, 1], s, None, None, 1, 3)[1] == 3      # label 2
    assert _device(cuda, y, s, None, None, 1, 3, dom=[0, 1, 0, 1, 2], n_domain=2)[1] == 5


def test_paired_vectors_share_the_weights(cuda):
    n, n_cluster, n_rep, y, s, sb, dom, cluster, uw, want, want_b, want_rows = _shared()
    same = _device(cuda, y, s, cluster, n_cluster, 77, n_rep, dom, 3, sb=s.copy())[0]
    for k in ("auc", "loss", "gauc"):
        assert _bits(same, {k: same[k + "_b"]}, (k,)), k                    # identical replicate matrices: every delta is 0
    got = _device(cuda, y, s, cluster, n_cluster, 77, n_rep, dom, 3, sb=sb)
    _check(got, want[False], "paired a")
    _check(got, want_b, "paired b", suffix="_b")
    assert not _bits(got[0], {"auc": got[0]["auc_b"]}, ("auc",))


def test_row_order_and_seed(cuda):
    n, n_cluster, n_rep, y, s, sb, dom, cluster, uw, want, want_b, want_rows = _shared()
    got = _device(cuda, y, s, cluster, n_cluster, 77, n_rep, dom, 3)
    again = _device(cuda, y, s, cluster, n_cluster, 77, n_rep, dom, 3)
    assert _bits(got[0], again[0])                                          # the same seed twice: the same bits everywhere
    perm = np.random.default_rng(1).permutation(n)
    moved = _device(cuda, y[perm], s[perm], cluster[perm], n_cluster, 77, n_rep, dom[perm], 3)
    assert _bits(got[0], moved[0], ("auc", "w_rows", "w_pos"))              # integer figures: order-free
    assert np.array_equal(np.isnan(got[0]["gauc"]), np.isnan(moved[0]["gauc"]))
    _check(moved, want[False], "permuted")                                  # loss and gauc inside their bounds
    other = _device(cuda, y, s, cluster, n_cluster, 78, n_rep, dom, 3)
    assert not _bits(got[0], other[0], ("w_rows",)) and not _bits(got[0], other[0], ("auc",))


def _delong_input():
    rng = np.random.default_rng(12)
    n = 600
    y = rng.integers(0, 2, n)
    s = (y * 0.8 + rng.normal(size=n)).astype(np.float32)
    return y, s


def test_row_bootstrap_spread_agrees_with_delong(cuda):
    """one row per cluster: the bootstrap's standard error of the AUC over 400 replicates against DeLong's on the same rows.  The band
    [0.8, 1.25] is the sampling noise of a standard deviation from 400 draws (about 3.5 % per sigma) widened for the bootstrap's own
    bias at n = 600; on the CPU the reference alone (bootstrap_sorted, seed 0, this input) gives se_boot / se_delong = 0.998."""
    from cdcmdr_amd.evaluate import eval_auc_ci, eval_bootstrap, summarize_bootstrap
    y, s = _delong_input()
    label = torch.from_numpy(y.astype(np.int16)).to(cuda)
    boot = eval_bootstrap(_f32(cuda, s), label, n_rep=400, seed=0)
    se, lo, hi, valid = summarize_bootstrap(boot.auc)
    assert se.is_cuda and valid.tolist() == [400, 400]
    ci = eval_auc_ci(_f32(cuda, s), label)
    ratio = (se / ci.var.sqrt()).cpu().tolist()
    print("se_boot / se_delong", ratio)
    assert all(0.8 <= v <= 1.25 for v in ratio)
    auc = ci.auc.cpu().tolist()
    assert lo[1].item() < auc[1] < hi[1].item()


def test_evaluator_bootstrap(cuda):
    from cdcmdr_amd.evaluate import Evaluator, eval_bootstrap, summarize_bootstrap
    model, loader, X, y = _tiny(cuda)
    w = {0: 0.5, 1: 0.3, 2: 0.2}
    kw = dict(mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w, user_idx=2, n_user=40)
    base = Evaluator(model, **kw)
    res0 = base.test(loader)
    assert sorted(res0) == ["domain_auc", "domain_gauc", "domain_loss", "mean_auc", "mean_gauc", "mean_loss", "total_auc", "total_gauc",
                            "total_loss"]                      # bootstrap=None: the parent's keys
    ev = Evaluator(model, bootstrap=16, bootstrap_seed=5, bootstrap_level=0.9, **kw)
    res = ev.test(loader)
    new = [f"{scope}_{name}_boot_{what}" for scope in ("total", "domain", "mean") for name in ("auc", "loss", "gauc")
           for what in ("se", "lo", "hi")]
    assert sorted(res) == sorted(list(res0) + new + ["boot_valid"])
    for k in res0:
        assert res[k] == res0[k]                                # the other figures are untouched
    pred, label, dom, user = ev._score(loader)
    boot = eval_bootstrap(pred, label, user, 40, dom, 3, 16, 5)
    wv = torch.tensor([w[d] for d in range(3)], dtype=torch.float64, device=cuda)
    valid = []
    for name in ("auc", "loss", "gauc"):
        reps = getattr(boot, name)
        mean = (reps[:, :3] * wv).sum(1)                        # formed per replicate
        se, lo, hi, ok = (t.cpu().tolist() for t in summarize_bootstrap(torch.cat([reps, mean[:, None]], 1), 0.9))
        valid += ok
        for what, v in (("se", se), ("lo", lo), ("hi", hi)):
            assert res[f"total_{name}_boot_{what}"] == v[3] and res[f"mean_{name}_boot_{what}"] == v[4], (name, what)
            assert res[f"domain_{name}_boot_{what}"] == {d: v[d] for d in range(3)}
        assert res[f"total_{name}_boot_se"] > 0 and res[f"total_{name}_boot_lo"] < res[f"total_{name}_boot_hi"]
        assert res[f"mean_{name}_boot_se"] > 0                  # mean_gauc's error, where mean_gauc_se cannot be offered
    assert res["boot_valid"] == min(valid) and 2 <= res["boot_valid"] <= 16
    # rows as clusters without a user column, per-domain evaluation off: the totals only
    res = Evaluator(model, mode="multi", domain_idx=3, n_domain=3, is_evaluate_multi_domain=False, bootstrap=8).test(loader)
    assert sorted(res) == sorted(["total_auc", "total_loss", "boot_valid"] +
                                 [f"total_{n}_boot_{x}" for n in ("auc", "loss") for x in ("se", "lo", "hi")])
    rows = eval_bootstrap(pred, label, n_rep=8)
    assert res["total_auc_boot_se"] == summarize_bootstrap(rows.auc)[0][1].item()

    # compare(): per-replicate differences under shared weights
    nine = ["domain_delta", "domain_delta_se", "domain_z", "mean_delta", "mean_delta_se", "mean_z", "total_delta", "total_delta_se", "total_z"]
    assert sorted(base.compare(base, loader)) == nine           # bootstrap=None: the parent's keys
    self_cmp = ev.compare(ev, loader)
    boot_keys = [f"{scope}_delta_boot_{what}" for scope in ("total", "domain", "mean") for what in ("se", "lo", "hi")]
    assert sorted(self_cmp) == sorted(nine + boot_keys + ["boot_valid"])
    assert self_cmp["total_delta_boot_se"] == 0.0 and self_cmp["mean_delta_boot_se"] == 0.0
    assert all(v == 0.0 for v in self_cmp["domain_delta_boot_se"].values())
    recal = base.fit_recalibration(loader, method="platt")
    other = Evaluator(model, recalibration=recal, **kw)
    full = Evaluator(model, bootstrap=16, bootstrap_seed=5, loss_ci=True, gauc_ci=True, **kw)
    both = full.compare(other, loader)
    for stem in ("delta", "loss_delta", "gauc_delta"):
        for scope in ("total", "domain", "mean"):
            for what in ("se", "lo", "hi"):
                assert f"{scope}_{stem}_boot_{what}" in both
    pb = other.predict(loader)[0]
    pair = eval_bootstrap(pred, label, user, 40, dom, 3, 16, 5, pred_b=pb)
    d_loss = pair.loss - pair.loss_b
    se = summarize_bootstrap(d_loss)[0].cpu().tolist()
    assert both["total_loss_delta_boot_se"] == se[3] > 0 and both["domain_loss_delta_boot_se"] == {d: se[d] for d in range(3)}
    assert both["mean_loss_delta_boot_se"] == summarize_bootstrap((d_loss[:, :3] * wv).sum(1))[0].item()
    assert both["mean_gauc_delta_boot_se"] == summarize_bootstrap(((pair.gauc - pair.gauc_b)[:, :3] * wv).sum(1))[0].item()
    assert both["total_delta_boot_lo"] <= both["total_delta_boot_hi"]
    # a loader that yields other rows on its second pass still raises
    class Shuffling:
        def __init__(self):
            self.calls = 0

        def __iter__(self):
            self.calls += 1
            return iter(loader if self.calls == 1 else loader[::-1])
    with pytest.raises(ValueError, match="different labels"):
        ev.compare(ev, Shuffling())
    # clusters are users: the other evaluator must see the same user column
    with pytest.raises(ValueError, match="different user columns"):
        ev.compare(Evaluator(model, mode="multi", domain_idx=3, n_domain=3, domain_cnt_weight=w), loader)
