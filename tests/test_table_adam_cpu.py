"""CPU-only checks around the lazy table's Adam replay: the host-built constants of the scaled fast replay
(optim.replay_constants) against values recorded before they were moved out of FusedAdam.__init__, the references of
tests/table_adam_ref.py against each other and against the oracle, the measurement of the fast path's margin K_FAST from those
references, and the proof that each seeded defect of the emulation breaks the bound the GPU tests assert."""
import math
import os

import numpy as np
import pytest
import torch

import table_adam_ref as T
from helpers import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALED = ("scaled", "scaled_l2_0")


# ----------------------------------------------------------------------------------------------------------------------
# (a) replay_constants returns what FusedAdam.__init__ built for the default hyper-parameters, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def test_replay_constants_equal_the_recorded_defaults_bit_for_bit():
    from cdcmdr_amd.optim import replay_constants, step_scalar_table
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))  # noqa: E731
    tab = step_scalar_table(1e-3, 0.9, 0.99, n=65536, truncate=True)
    assert tab.shape == (1657, 2)
    rc = replay_constants(tab, f32(1.0 - 0.9), f32(1.0 - 0.99), f32(1e-8), f32(1e-8), 1e-5)
    want = {"k1": "0x1.0c91d60000000p-19", "k2": "0x1.19c1ac0000000p-38", "ik1": "0x1.e809880000000p+18", "ik2": "0x1.d1322a0000000p+37",
            "k1_lo": "0x1.14f7b40000000p-46", "k2_lo": "0x1.285ade0000000p-64"}
    for k, h in want.items():
        assert float(getattr(rc, k)).hex() == h, k
    gold = np.load(os.path.join(ROOT, "tests", "golden", "table_adam_replay_tab.npz"))
    assert rc.replay_tab.dtype == torch.float32 and rc.replay_tab.is_contiguous() and rc.inv_bc2.dtype == torch.float32
    assert_bits_equal(rc.replay_tab.numpy(), gold["replay_tab"], "replay_tab")
    assert_bits_equal(rc.inv_bc2.numpy(), gold["inv_bc2"], "inv_bc2")


def test_replay_constants_without_a_decay_term_have_no_scaled_form():
    hp = T.hp_of(0.0, 0.0)
    assert hp.rc.replay_tab is None and (hp.rc.k1, hp.rc.k2, hp.rc.ik1, hp.rc.ik2, hp.rc.k1_lo, hp.rc.k2_lo) == (0.0,) * 6
    assert hp.rc.inv_bc2.shape == (hp.last_i + 1,)
    for mode in SCALED:
        rc = T.hp_of(*T.MODES[mode][1:]).rc
        assert rc.replay_tab is not None and rc.k1 > 0 and rc.k2 > 0
        # in and out scales are inverses far below fp32 resolution
        assert abs((rc.k1 + rc.k1_lo) * rc.ik1 - 1.0) < 2.0 ** -45 and abs((rc.k2 + rc.k2_lo) * rc.ik2 - 1.0) < 2.0 ** -45


def test_the_matrix_straddles_the_end_of_the_step_scalar_table():
    hp = T.hp_of(1e-8, 1e-5)
    tab = hp.tab
    # the truncated table ends with the first row at the fp32 limits of both columns: the steps past it read that row
    assert hp.last_i == 1656 and tuple(tab[hp.last_i]) == (np.float32(1e-3), np.float32(1.0)) and not (tab[hp.last_i] == tab[hp.last_i - 1]).all()
    tg = T.targets(hp)
    assert min(tg) == 1 and sum(t < hp.last_i for t in tg) >= 4 and hp.last_i in tg and sum(t > hp.last_i for t in tg) == 2
    for mode in T.MODES:
        mx = T.matrix(mode)
        assert len(mx) == 3 * 3 + 4 * 2 and all(s != "fresh" or t <= T.SHALLOW for t, s in mx)
    c = T.case("scaled", hp.last_i + 300, "trained")
    assert set(np.unique(c.last)) == {0, 1, 3, hp.last_i + 299, hp.last_i + 300, hp.last_i + 301, (hp.last_i + 300) // 2}
    for r0 in range(0, T.ROWS, 16):                                # 16 rows of D = 16: one wave of a flush
        assert len(np.unique(c.last[r0:r0 + 16])) >= 3, "every wave mixes start steps"


# ----------------------------------------------------------------------------------------------------------------------
# (b) the references against the oracle and against each other
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 5, 2000])
def test_replay_f64_over_one_step_is_the_oracles_adam_step(step, monkeypatch):
    from oracle import cdc_oracle as O
    hp = T.hp_of(1e-8, 1e-5)
    rng = np.random.default_rng(step)
    w, m = rng.standard_normal((7, 5)) * 0.1, rng.standard_normal((7, 5)) * 1e-3
    v = rng.random((7, 5)) * 1e-6
    got = T.replay_f64(w, m, v, step - 1, step, hp)
    tw, tm, tv = (torch.from_numpy(a) for a in (w, m, v))
    # zero batch gradient plus the L2 term.  The oracle forms its step scalars in double from the step number, the kernels read
    # them from the fp32 table: the oracle is handed the table's values, which agree with its own to fp32 rounding
    ss, bc = (float(x) for x in hp.scalars(step))
    ss64, bc64 = O.adam_scalars(step, 1e-3, 0.9, 0.99)
    assert abs(ss / ss64 - 1) <= 2.0 ** -24 and abs(bc / bc64 - 1) <= 2.0 ** -24
    monkeypatch.setattr(O, "adam_scalars", lambda *a, **k: (ss, bc))
    want = O.adam_step(tw, hp.l2_twice * tw, tm, tv, step, lr=1e-3, beta1=1.0 - hp.lerp_w, beta2=hp.beta2, eps=hp.eps, weight_decay=hp.wd)
    # the one constant the two do not share: the oracle takes 1 - beta2 in double, the kernels get its fp32 rounding — that moves
    # v by d_omb2 * g^2 and the weight's update by at most the same relative amount
    xw, xm, xv = (x.numpy() for x in want)
    slack_v = abs(hp.omb2 - (1.0 - hp.beta2)) * ((hp.l2_twice + hp.wd) * w) ** 2
    slack = {"w": np.abs(xw - w) * slack_v / xv, "m": 0.0, "v": slack_v}
    for q, g, x in zip("wmv", got, (xw, xm, xv)):
        assert x.dtype == np.float64 and (np.abs(g - x) <= 1e-14 * np.abs(x) + slack[q]).all(), q
        assert (x != {"w": w, "m": m, "v": v}[q]).all()
    rows = np.array([step - 1, step, step + 1, step - 1, 0, step, step - 1])
    part = T.replay_f64(w, m, v, rows, step, hp)
    for g, p, a in zip(got, part, (w, m, v)):
        sel = rows == step - 1
        assert np.array_equal(p[sel], g[sel]) and np.array_equal(p[rows >= step], a[rows >= step])


def test_replay_c32_is_repeated_calls_of_the_c_restatement():
    from test_host_logic import _build_adam_ref
    lib = _build_adam_ref()
    hp = T.hp_of(1e-8, 1e-5)
    rng = np.random.default_rng(3)
    n, to = 40, hp.last_i + 3
    w, m = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32), (rng.standard_normal((n, 3)) * 1e-3).astype(np.float32)
    v = (rng.random((n, 3)) * 1e-6).astype(np.float32)
    frm = rng.choice([0, 2, hp.last_i - 2, to - 1, to, to + 1], size=n)
    got = T.replay_c32(w, m, v, frm, to, hp)
    zero = np.zeros(3, np.float32)
    for r in range(n):
        a, b, c = w[r].copy(), m[r].copy(), v[r].copy()
        for s in range(int(frm[r]) + 1, to + 1):
            i = min(s, hp.last_i)
            lib.adam_elem_ref(a.ctypes.data, b.ctypes.data, c.ctypes.data, zero.ctypes.data, 3, hp.lerp_w, hp.beta2, hp.omb2, hp.eps, hp.wd,
                              hp.l2_twice, float(hp.tab[i, 0]), float(hp.tab[i, 1]))
        for g, x, nm in zip(got, (a, b, c), "wmv"):
            assert_bits_equal(g[r], x, f"row {r} {nm}")
    for g, x in zip(got, (w, m, v)):
        assert_bits_equal(g[frm >= to], x[frm >= to], "rows at or past the target")
    assert math.isfinite(float(np.abs(got[0]).max()))


# ----------------------------------------------------------------------------------------------------------------------
# (c) K_FAST measured from references only, (d) every seeded defect exceeds the fast bound
# ----------------------------------------------------------------------------------------------------------------------
def _measure():
    worst = {q: (0.0, None) for q in "wmv"}
    for mode in SCALED:
        for t, s in T.matrix(mode):
            c = T.case(mode, t, s)
            got = T.replay_scaled_emulated(c.w0, c.m0, c.v0, c.last, t, c.hp, rng=np.random.default_rng([t, T.STATES.index(s)]))
            r = T.check(got, c, T.K_FAST, what=f"emulation {mode} target {t} {s}")
            for q in "wmv":
                if r[q] > worst[q][0]:
                    worst[q] = (r[q], (mode, t, s))
    return worst


def test_k_fast_is_twice_the_emulations_worst_ratio_rounded_up_to_a_power_of_two():
    worst = _measure()
    for q in "wmv":
        print(f"emulated scaled replay, +-1 ulp sqrt/rcp: worst {q} error / E_ref = {worst[q][0]:.2f} at {worst[q][1]}")
        assert math.isfinite(worst[q][0]) and worst[q][0] > 0
        assert worst[q][0] < T.K_FAST[q] / 2, (q, worst[q])
        assert T.K_FAST[q] == 2.0 ** math.ceil(math.log2(2 * worst[q][0])), (q, worst[q], T.K_FAST[q])
    assert all(k == 4.0 for k in T.K_EXACT.values())


def test_the_unperturbed_emulation_leaves_finished_rows_alone():
    c = T.case("scaled", 8, "trained")
    got = T.replay_scaled_emulated(c.w0, c.m0, c.v0, c.last, 8, c.hp)
    keep = c.last >= 8
    assert keep.sum() >= 2 and (~keep).sum() > 100
    for g, x in zip(got, (c.w0, c.m0, c.v0)):
        assert_bits_equal(g[keep], x[keep], "rows at or past the target")
        assert (g[~keep] != x[~keep]).any()


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_each_seeded_defect_exceeds_the_fast_bound(defect):
    """over the shallow half of the matrix (the shifted table index is visible only while a row starts below step ~20: every case
    holds rows that start at 0, 1 and 3)"""
    caught, ran = [], 0
    for mode in SCALED:
        for t, s in T.matrix(mode):
            if t > T.SHALLOW:
                continue
            c = T.case(mode, t, s)
            got = T.replay_scaled_emulated(c.w0, c.m0, c.v0, c.last, t, c.hp, defect=defect)
            if got is None:
                continue
            ran += 1
            try:
                T.check(got, c, T.K_FAST)
            except AssertionError:
                caught.append((mode, t, s))
    print(f"defect {defect}: exceeds the bound in {len(caught)} of {ran} cases")
    assert caught, f"defect {defect} passes the fast bound in all {ran} cases"
    if defect in ("short", "long", "shift"):
        assert len(caught) == ran                                   # a miscounted step shows at any depth and in any state


def test_a_shifted_table_index_is_invisible_to_rows_that_start_late():
    """why every case holds rows with last in {0, 1, 3}: the same defect on rows that all start at step 1600 stays within the bound"""
    c = T.case("scaled", T.hp_of(1e-8, 1e-5).last_i + 300, "trained")
    frm = np.full(T.ROWS, 1600, dtype=np.int32)
    to = 1700
    f64, c32 = T.replay_f64(c.w0, c.m0, c.v0, frm, to, c.hp), T.replay_c32(c.w0, c.m0, c.v0, frm, to, c.hp)
    late = c._replace(last=frm, target=to, f64=f64, c32=c32)
    T.check(T.replay_scaled_emulated(c.w0, c.m0, c.v0, frm, to, c.hp, defect="shift"), late, T.K_FAST)
    with pytest.raises(AssertionError):
        T.check(T.replay_scaled_emulated(c.w0, c.m0, c.v0, frm, to, c.hp, defect="short"), late, T.K_FAST)
