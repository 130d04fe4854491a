"""The lazy table's Adam replay, flush and catch-up launches, and the dense form's three launches (csrc/embedding.hip, csrc/common.h),
straight through the C-ABI against the float64 recurrence of tests/table_adam_ref.py.

Bounds come from references only: a path may deviate from float64 by K * E_ref + floor, E_ref being the deviation of the fp32
C restatement from float64 on the same elements (table_adam_ref.bounds); K_EXACT = 4 for the exact routine, K_FAST as measured on the
CPU by tests/test_table_adam_cpu.py for every fast form.  The AdamHP comes from optim.replay_constants, so the host-built table of the
scaled replay is under test together with the kernels.  Every table sits between guard rows (last = 0: a launch that strays into
them replays them) inside a buffer whose every other element must come back bit for bit, and every launch is followed by a
check that the rows outside its scope kept w, m, v and last bit for bit.

  A  replay arithmetic through cdc_embed_lazy_flush (period 0): D x alignment x mode x target x state, on both sides of the end
     of the step-scalar table; scalar path (D = 6, misaligned D = 8), mark == 0 (D = 12), unscaled fast path (no decay term)
  B  which rows a sliced / sharded flush may touch, foreground against background launch
  C  cdc_embed_lazy_catchup and cdc_embed_lazy_catchup_gather: values, the three routes bit for bit, the gathered rows and
     their bf16 shadow, the 4|5 and 32|33 segment-length boundaries, argument checks
  D  cdc_embed_adam_touched -> cdc_embed_adam_dense_pass -> cdc_embed_adam_patch: scalar tail, second grid-stride trip, reg_sum
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import table_adam_ref as T
from helpers import assert_bits_equal, assert_bounded, sum_bound

pytestmark = pytest.mark.gpu

BADARG, ALIGN = -1, -3
GUARD = 4                               # guard rows in front of and behind every table (4 rows: 16 D bytes, alignment is kept)
BF16_SENTINEL = -776.0                  # exact in bf16


@pytest.fixture(scope="module")
def lib(cuda):
    from cdcmdr_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    from cdcmdr_amd import _lib as L
    L.check(getattr(lib, name)(*args, _stream()), name)


def _dev(cuda, a):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)


class DevHP:
    """cdc_adam_hp as FusedAdam._hp fills it, from table_adam_ref.HP (= optim.step_scalar_table + optim.replay_constants)"""

    def __init__(self, cuda, fast, wd, l2):
        from cdcmdr_amd import _lib as L
        h = T.hp_of(wd, l2)
        self.h, self.fast = h, fast
        self.scalars = h.tab_t.to(cuda).contiguous()
        self.inv_bc2 = h.rc.inv_bc2.to(cuda).contiguous()
        self.replay_tab = h.rc.replay_tab.to(cuda).contiguous() if (fast and h.rc.replay_tab is not None) else None
        hp = L.AdamHP()
        hp.lerp_w, hp.beta2, hp.one_minus_beta2, hp.eps = h.lerp_w, h.beta2, h.omb2, h.eps
        hp.weight_decay, hp.l2_twice = h.wd, h.l2_twice
        hp.step_scalars, hp.n_scalars = self.scalars.data_ptr(), self.scalars.shape[0]
        hp.fast_replay = 1 if fast else 0
        hp.inv_bc2 = self.inv_bc2.data_ptr()
        hp.replay_tab = None
        if self.replay_tab is not None:
            hp.replay_tab = self.replay_tab.data_ptr()
            hp.k1, hp.k2, hp.ik1, hp.ik2, hp.k1_lo, hp.k2_lo = h.rc.k1, h.rc.k2, h.rc.ik1, h.rc.ik2, h.rc.k1_lo, h.rc.k2_lo
        self.c = hp


_HP = {}


def dev_hp(cuda, mode):
    if mode not in _HP:
        _HP[mode] = DevHP(cuda, *T.MODES[mode])
    return _HP[mode]


class Table:
    """w, m, v [R, D] and last [R] on the device between GUARD rows, `offset` floats into buffers filled with finite noise;
    read() returns the table and asserts that everything around it came back bit for bit."""

    def __init__(self, cuda, w, m, v, last, offset=0):
        self.R, self.D = w.shape
        R, D = w.shape
        rng = np.random.default_rng(R * 1000 + D)
        n = offset + (R + 2 * GUARD) * D + 5
        self.lo, self.hi = offset + GUARD * D, offset + (GUARD + R) * D
        noise = (0.05 * rng.standard_normal(n), 1e-3 * rng.standard_normal(n), rng.uniform(1e-8, 1e-6, n))
        self.host, self.bufs = [], []
        for a, g in zip((w, m, v), noise):
            h = g.astype(np.float32)
            h[self.lo:self.hi] = np.asarray(a, dtype=np.float32).reshape(-1)
            self.host.append(h)
            self.bufs.append(torch.from_numpy(h.copy()).to(cuda))
        self.last_host = np.zeros(R + 2 * GUARD, dtype=np.int32)
        self.last_host[GUARD:GUARD + R] = last
        self.last_buf = torch.from_numpy(self.last_host.copy()).to(cuda)
        self.w, self.m, self.v = (b.data_ptr() + 4 * self.lo for b in self.bufs)
        self.last = self.last_buf.data_ptr() + 4 * GUARD
        assert (self.w % 16 == 0) == (offset % 4 == 0)

    @property
    def args(self):
        return self.w, self.m, self.v, self.last

    def read(self, what=""):
        out = []
        for b, h, nm in zip(self.bufs, self.host, "wmv"):
            g = b.cpu().numpy()
            keep = np.ones(g.size, dtype=bool)
            keep[self.lo:self.hi] = False
            assert np.array_equal(g[keep].view(np.int32), h[keep].view(np.int32)), f"{what}: {nm} written outside the table"
            out.append(g[self.lo:self.hi].reshape(self.R, self.D).copy())
        la = self.last_buf.cpu().numpy()
        assert (la[:GUARD] == 0).all() and (la[GUARD + self.R:] == 0).all(), f"{what}: last[] written outside the table"
        return out[0], out[1], out[2], la[GUARD:GUARD + self.R].copy()


def assert_rows_kept(got, w0, m0, v0, last0, keep, what):
    """rows `keep` (bool [R]) hold their inputs bit for bit, last included"""
    for g, a, nm in zip(got[:3], (w0, m0, v0), "wmv"):
        assert_bits_equal(g[keep], np.asarray(a)[keep], f"{what}: {nm} of rows outside the call's scope")
    assert np.array_equal(got[3][keep], np.asarray(last0)[keep]), f"{what}: last of rows outside the call's scope"


def assert_tables_equal(a, b, what, rows=None):
    sel = slice(None) if rows is None else rows
    for x, y, nm in zip(a[:3], b[:3], "wmv"):
        assert_bits_equal(x[sel], y[sel], f"{what}: {nm}")
    assert np.array_equal(a[3][sel], b[3][sel]), f"{what}: last"


def _step(cuda, t):
    return torch.full((1,), int(t), dtype=torch.int32, device=cuda)


def _flush(lib, tab, hp, step, bias=0, period=0, own_mod=0, own_rem=0, bg=0):
    if bg:
        call(lib, "cdc_embed_lazy_flush_bg", *tab.args, tab.R, tab.D, hp.c, step.data_ptr(), bias, period, own_mod, own_rem, bg)
    else:
        call(lib, "cdc_embed_lazy_flush", *tab.args, tab.R, tab.D, hp.c, step.data_ptr(), bias, period, own_mod, own_rem)


# ------------------------------------------------------------------------------------------------------------------------
# A. replay arithmetic through cdc_embed_lazy_flush
# ------------------------------------------------------------------------------------------------------------------------
DCFG = [(4, 0), (6, 0), (8, 1), (12, 0), (32, 0), (256, 0)]      # (D, table pointers offset by this many floats)


def _cases(mode, D):
    return [(t, s) for t, s in T.matrix(mode) if t <= T.SHALLOW or D <= T.COLS_DEEP]


def _run_flush_case(cuda, lib, mode, D, off, target, state):
    c = T.case(mode, target, state)
    hp = dev_hp(cuda, mode)
    tab = Table(cuda, c.w0[:, :D], c.m0[:, :D], c.v0[:, :D], c.last, off)
    _flush(lib, tab, hp, _step(cuda, target))
    return c, tab.read(f"flush {mode} D {D}+{off} target {target} {state}")


@pytest.mark.parametrize("mode", list(T.MODES))
@pytest.mark.parametrize("D,off", DCFG, ids=[f"D{d}" + ("_offset" if o else "") for d, o in DCFG])
def test_flush_replay_against_float64(cuda, lib, D, off, mode):
    """Rows with mixed start steps inside every wave brought to `target`: w, m, v within K * E_ref + floor of float64, last = target;
    rows already at target or past it bit-identical with last unchanged.  Targets straddle the last row of the step-scalar table."""
    hp = dev_hp(cuda, mode)
    fast, h = T.MODES[mode][0], hp.h
    assert (hp.replay_tab is not None) == mode.startswith("scaled") and (h.rc.replay_tab is None) == (mode == "unscaled")
    tg = [t for t, _ in _cases(mode, D)]
    if D <= T.COLS_DEEP:
        assert h.last_i - 1 in tg and h.last_i in tg and h.last_i + 1 in tg and max(tg) == h.last_i + 300
    K = T.K_FAST if fast else T.K_EXACT
    worst = {q: 0.0 for q in "wmv"}
    for target, state in _cases(mode, D):
        c, got = _run_flush_case(cuda, lib, mode, D, off, target, state)
        what = f"flush {mode} D {D}+{off} target {target} {state}"
        keep = c.last >= target
        assert keep.sum() >= 2 and (~keep).sum() >= 50
        assert_rows_kept(got, c.w0[:, :D], c.m0[:, :D], c.v0[:, :D], c.last, keep, what)
        assert (got[3][~keep] == target).all(), f"{what}: last of the replayed rows"
        r = T.check(got[:3], c, K, cols=D, what=what)
        if (mode, state) != ("unscaled", "fresh"):                    # (no decay term and zero moments: the steps leave w where it is)
            assert (got[0][~keep] != c.w0[:, :D][~keep]).any(), f"{what}: the replayed rows did not move"
        for q in "wmv":
            worst[q] = max(worst[q], r[q])
    print(f"\nflush replay, mode {mode}, D {D}+{off}: worst error / E_ref  w {worst['w']:.2f}  m {worst['m']:.2f}  v {worst['v']:.2f}  (K {K['w']:g})")


@pytest.mark.parametrize("D", [4, 8, 12, 32, 256])
def test_exact_flush_bits_do_not_depend_on_alignment(cuda, lib, D):
    """adam_elem is the same routine on the 16-byte path and on the scalar path a misaligned table takes"""
    for target, state in _cases("exact", D):
        _, a = _run_flush_case(cuda, lib, "exact", D, 0, target, state)
        _, b = _run_flush_case(cuda, lib, "exact", D, 1, target, state)
        assert_tables_equal(a, b, f"exact flush D {D} target {target} {state}: aligned against offset by one float")


# ------------------------------------------------------------------------------------------------------------------------
# B. which rows a flush may touch
# ------------------------------------------------------------------------------------------------------------------------
def _slice_rows(R, period, target):
    rows = np.arange(R)
    if period <= 1:
        return np.ones(R, dtype=bool)
    rps = -(-R // period)
    sl = ((target % period) + period) % period
    return (rows >= sl * rps) & (rows < min(sl * rps + rps, R))


def _flush_set(R, period, target, own_mod, own_rem, last):
    """the kernel's documented rule: slice ((target % period) + period) % period of ceil(R / period) rows, owned rows only, last < target"""
    owned = (np.arange(R) % own_mod == own_rem) if own_mod > 1 else np.ones(R, dtype=bool)
    return _slice_rows(R, period, target) & owned & (np.asarray(last) < target)


@pytest.mark.parametrize("mode", ["exact", "scaled"])
@pytest.mark.parametrize("R,period,D", [(50, 3, 8), (50, 8, 8), (10, 3, 8), (10, 8, 8), (50, 8, 12), (10, 3, 12)])
def test_flush_touches_exactly_its_slice(cuda, lib, R, period, D, mode):
    """period > 1 with R not divisible by it, empty trailing slices, step_bias 0 and -1 (a negative target changes nothing),
    own_mod / own_rem sharding inside slices, rows at or past the target; the background launch equals the foreground one.
    D = 12: last[] is advanced by k_lazy_set_last."""
    hp = dev_hp(cuda, mode)
    K = T.K_FAST if hp.fast else T.K_EXACT
    rng = np.random.default_rng(R * 100 + period * 10 + D)
    w0 = (0.01 * rng.standard_normal((R, D))).astype(np.float32)
    m0 = (1e-3 * rng.standard_normal((R, D))).astype(np.float32)
    v0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e-6), size=(R, D))).astype(np.float32)
    last0 = rng.integers(0, 16, size=R).astype(np.int32)
    base = 5
    sizes = sorted(int(_slice_rows(R, period, t).sum()) for t in range(period))
    if (R, period) == (10, 8):
        assert sizes == [0, 0, 0, 2, 2, 2, 2, 2]                    # slices 5..7 are empty
    if (R, period) == (50, 8):
        assert sizes[0] == 1                                        # a one-row last slice
    runs = [(s, b) for b in (0, -1) for s in range(base, base + period)] + [(0, -1)]
    for b in (0, -1):
        assert sorted((s + b) % period for s, bb in runs[:-1] if bb == b) == list(range(period))     # every slice index once
    touched_any = False
    for own_mod in (0, 3):
        for own_rem in range(max(own_mod, 1)):
            for step, bias in runs:
                target = step + bias
                sel = _flush_set(R, period, target, own_mod, own_rem, last0)
                what = f"flush R {R} D {D} period {period} step {step} bias {bias} own {own_rem}/{own_mod} ({mode})"
                if target < 0:
                    assert not sel.any()
                touched_any |= bool(sel.any())
                c = T.custom_case(hp.h, w0, m0, v0, np.where(sel, last0, max(target, 0)), max(target, 0))
                fg, bg = Table(cuda, w0, m0, v0, last0), Table(cuda, w0, m0, v0, last0)
                sd = _step(cuda, step)
                _flush(lib, fg, hp, sd, bias, period, own_mod, own_rem)
                _flush(lib, bg, hp, sd, bias, period, own_mod, own_rem, bg=1)
                got, got_bg = fg.read(what), bg.read(what + " background")
                assert_tables_equal(got_bg, got, what + ": background against foreground launch")
                assert_rows_kept(got, w0, m0, v0, last0, ~sel, what)
                assert (got[3][sel] == target).all(), f"{what}: last of the flushed rows"
                T.check(got[:3], c, K, what=what)
                if sel.any():
                    assert (got[0][sel] != w0[sel]).any()
    assert touched_any


# ------------------------------------------------------------------------------------------------------------------------
# C. catch-up of a batch's rows, alone and fused with the gather
# ------------------------------------------------------------------------------------------------------------------------
CG_F, CG_R = 4, 500
CG_LENS = [33, 32, 5, 4, 1, 33, 32, 5, 4, 1, 17, 16, 8, 6, 3]     # field 1: both sides of the inline (4|5) and the hot (32|33) boundary


@functools.lru_cache(maxsize=None)
def _batch(B):
    """[B, 4] table rows: field 0 three hot rows, field 1 the segment lengths CG_LENS, field 2 all distinct, field 3 with ids of -1"""
    rng = np.random.default_rng(B)
    idx = np.empty((B, CG_F), dtype=np.int32)
    if B == 1:
        idx[0] = (2, 17, 300, -1)
        return idx
    assert sum(CG_LENS) == B
    idx[:, 0] = rng.permutation(np.arange(B) % 3)
    idx[:, 1] = rng.permutation(np.repeat(3 + rng.permutation(40)[:len(CG_LENS)], CG_LENS))
    idx[:, 2] = 43 + rng.permutation(400)[:B]
    idx[:, 3] = 443 + rng.integers(0, 40, size=B)
    idx[rng.permutation(B)[:9], 3] = -1
    idx.setflags(write=False)
    return idx


def _sort(cuda, lib, idx):
    B, F = idx.shape
    d_idx = _dev(cuda, idx)
    uniq = torch.full((F, B), -7, dtype=torch.int32, device=cuda)
    seg = torch.full((F, B + 1), -7, dtype=torch.int32, device=cuda)
    perm = torch.full((F, B), -7, dtype=torch.int32, device=cuda)
    cnt = torch.zeros(F, dtype=torch.int32, device=cuda)
    call(lib, "cdc_embed_sort_dedupe", d_idx.data_ptr(), uniq.data_ptr(), seg.data_ptr(), perm.data_ptr(), cnt.data_ptr(), None, B, F)
    return uniq, seg, perm, cnt


@functools.lru_cache(maxsize=None)
def _cg_case(wd, l2, D, B, target):
    """table, start steps and references of a catch-up to `target`: only the batch's rows may move.  Most rows start one or two
    steps back, a few at 0, 1, 3 and half way, some are at the target already or past it."""
    hp = T.hp_of(wd, l2)
    rng = np.random.default_rng([D, B, target])
    w0 = (0.01 * rng.standard_normal((CG_R, D))).astype(np.float32)
    m0 = (1e-3 * rng.standard_normal((CG_R, D))).astype(np.float32)
    v0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e-6), size=(CG_R, D))).astype(np.float32)
    choice = np.array([0, 1, 3, target // 2, max(target - 2, 0), target - 1, target, target + 1], dtype=np.int32)
    last0 = choice[rng.choice(len(choice), size=CG_R, p=[0.02, 0.02, 0.02, 0.04, 0.2, 0.4, 0.25, 0.05])]
    idx = _batch(B)
    if B == 1:
        last0[idx[0, :3]] = (0, target - 1, target)
    in_batch = np.zeros(CG_R, dtype=bool)
    in_batch[idx[idx >= 0]] = True
    move = in_batch & (last0 < target)
    assert move.sum() >= min(B, 2) and (in_batch & ~move).sum() >= 1 and (~in_batch).sum() > 100
    c = T.custom_case(hp, w0, m0, v0, np.where(move, last0, target), target)
    return c, last0, in_batch, move


CG_SHAPES = [(4, 200), (16, 200), (256, 200), (16, 1), (256, 1)]


@pytest.mark.parametrize("deep", [False, True], ids=["step9", "past_table_end"])
@pytest.mark.parametrize("mode", ["exact", "scaled"])
@pytest.mark.parametrize("D,B", CG_SHAPES, ids=[f"D{d}_B{b}" for d, b in CG_SHAPES])
def test_catchup_gather_catchup_and_flush_agree_and_match_float64(cuda, lib, D, B, mode, deep):
    hp = dev_hp(cuda, mode)
    K = T.K_FAST if hp.fast else T.K_EXACT
    step = hp.h.last_i + 6 if deep else 9
    target = step - 1
    assert (target > hp.h.last_i) == deep
    c, last0, in_batch, move = _cg_case(*T.MODES[mode][1:], D, B, target)
    idx = _batch(B)
    F = CG_F
    uniq, seg, perm, cnt = _sort(cuda, lib, idx)
    if B > 1:
        lens = [np.diff(seg[f, :int(cnt[f]) + 1].cpu().numpy()) for f in range(F)]
        assert len(lens[0]) == 3 and lens[0].min() > 32                                 # hot rows
        assert {1, 4, 5, 32, 33} <= set(lens[1].tolist())                               # both sides of both boundaries
        assert int(cnt[2]) == B and (uniq[3, :int(cnt[3])] == -1).any()
    what = f"D {D} B {B} {mode} step {step}"
    sd = _step(cuda, step)
    ld_h = F * D + 8
    ta, tb, tc = (Table(cuda, c.w0, c.m0, c.v0, last0) for _ in range(3))
    out = torch.full((B, F * D), float("nan"), device=cuda)
    out_h = torch.full((B, ld_h), BF16_SENTINEL, dtype=torch.bfloat16, device=cuda)
    call(lib, "cdc_embed_lazy_catchup_gather", uniq.data_ptr(), cnt.data_ptr(), seg.data_ptr(), perm.data_ptr(), *ta.args, hp.c,
         sd.data_ptr(), out.data_ptr(), out_h.data_ptr(), ld_h, B, F, D)
    call(lib, "cdc_embed_lazy_catchup", uniq.data_ptr(), cnt.data_ptr(), *tb.args, hp.c, sd.data_ptr(), None, 0, B, F, D)
    _flush(lib, tc, hp, sd, bias=-1)
    ga, gb, gc = ta.read(what + " catchup_gather"), tb.read(what + " catchup"), tc.read(what + " flush")
    # the batch's rows against float64, every other row untouched
    assert_rows_kept(ga, c.w0, c.m0, c.v0, last0, ~move, what + " catchup_gather")
    assert (ga[3][move] == target).all()
    r = T.check(ga[:3], c, K, what=what + " catchup_gather")
    assert (ga[0][move] != c.w0[move]).any()
    # the three routes call one routine
    assert_tables_equal(gb, ga, what + ": catchup against catchup_gather")
    assert_tables_equal(gc, ga, what + ": flush against catchup_gather", rows=in_batch)
    assert (gc[3][last0 < target] == target).all()
    # the gathered rows
    o = out.cpu().numpy().reshape(B, F, D)
    assert not np.isnan(o).any(), f"{what}: positions of `out` left unwritten"
    want = np.where((idx >= 0)[:, :, None], ga[0][np.maximum(idx, 0)], np.float32(0.0))
    assert_bits_equal(o, want, what + ": out[b, f] against the table row after the call")
    assert (idx < 0).any() and (o[idx < 0] == 0).all()
    oh = out_h.cpu()
    assert torch.equal(oh[:, :F * D].view(torch.int16), out.cpu().to(torch.bfloat16).view(torch.int16)), f"{what}: bf16 shadow"
    assert (oh[:, F * D:].float() == BF16_SENTINEL).all(), f"{what}: bf16 shadow's padding written"
    print(f"\ncatchup_gather {what}: worst error / E_ref  w {r['w']:.2f}  m {r['m']:.2f}  v {r['v']:.2f}  (K {K['w']:g})")


@pytest.mark.parametrize("deep", [False, True], ids=["step9", "past_table_end"])
@pytest.mark.parametrize("mode", ["exact", "scaled"])
@pytest.mark.parametrize("D", [12, 6])
def test_catchup_without_a_fused_form(cuda, lib, D, mode, deep):
    """D = 12 (three 16-byte lanes per row: last[] advanced by k_lazy_mark) and D = 6 (scalar replay)"""
    hp = dev_hp(cuda, mode)
    K = T.K_FAST if hp.fast else T.K_EXACT
    B, F = 200, CG_F
    step = hp.h.last_i + 6 if deep else 9
    target = step - 1
    c, last0, in_batch, move = _cg_case(*T.MODES[mode][1:], D, B, target)
    uniq, seg, perm, cnt = _sort(cuda, lib, _batch(B))
    what = f"catchup D {D} {mode} step {step}"
    sd = _step(cuda, step)
    tb, tc = Table(cuda, c.w0, c.m0, c.v0, last0), Table(cuda, c.w0, c.m0, c.v0, last0)
    call(lib, "cdc_embed_lazy_catchup", uniq.data_ptr(), cnt.data_ptr(), *tb.args, hp.c, sd.data_ptr(), None, 0, B, F, D)
    _flush(lib, tc, hp, sd, bias=-1)
    gb, gc = tb.read(what), tc.read(what + " flush")
    assert_rows_kept(gb, c.w0, c.m0, c.v0, last0, ~move, what)
    assert (gb[3][move] == target).all(), f"{what}: last of the batch's rows"
    T.check(gb[:3], c, K, what=what)
    assert (gb[0][move] != c.w0[move]).any()
    assert_tables_equal(gc, gb, what + ": flush against catchup", rows=in_batch)


def test_catchup_gather_refuses_what_it_cannot_run(cuda, lib):
    hp = dev_hp(cuda, "exact")
    B, F = 200, CG_F
    uniq, seg, perm, cnt = _sort(cuda, lib, _batch(B))
    sd = _step(cuda, 9)

    def run(D, shift):
        c, last0, _, _ = _cg_case(*T.MODES["exact"][1:], D, B, 8)
        t = Table(cuda, c.w0, c.m0, c.v0, last0)
        out = torch.full((B, F * D), float("nan"), device=cuda)
        rc = lib.cdc_embed_lazy_catchup_gather(uniq.data_ptr(), cnt.data_ptr(), seg.data_ptr(), perm.data_ptr(), t.w + shift, t.m, t.v, t.last,
                                               hp.c, sd.data_ptr(), out.data_ptr(), None, 0, B, F, D, _stream())
        msg = lib.cdc_last_error()
        got = t.read(f"refused launch D {D}")
        assert_rows_kept(got, c.w0, c.m0, c.v0, last0, np.ones(CG_R, dtype=bool), f"refused launch D {D}")
        assert torch.isnan(out).all()
        return rc, msg

    rc, msg = run(12, 0)
    assert rc == BADARG and b"embed_lazy_catchup_gather: emb_dim must be 4, 8, 16, 32, 64, 128 or 256" in msg
    rc, msg = run(16, 4)
    assert rc == ALIGN and b"embed_lazy_catchup_gather: table and output must be 16-byte aligned" in msg


# ------------------------------------------------------------------------------------------------------------------------
# D. the dense form: touched rows to a side buffer, one pass over the whole table, the side buffer patched in
# ------------------------------------------------------------------------------------------------------------------------
DENSE = [(5, 3, 6, 3), (5, 3, 6, None), (419450, 5, 64, 7)]         # (R, D, B, step; None: past the end of the step-scalar table)


@pytest.mark.parametrize("R,D,B,step", DENSE, ids=["tail_step3", "tail_past_table_end", "second_grid_trip"])
def test_dense_form_one_step_against_float64(cuda, lib, R, D, B, step):
    """One Adam step of the whole table: R * D = 15 elements exercise the pass's scalar tail, 419450 * 5 = 2 097 250 elements
    (> 2048 blocks x 256 threads x 4) a second grid-stride trip and a tail of two.  Touched rows take their batch gradient,
    all others the L2-only step; reg_sum is the sum of squares of the weights before the step."""
    hp = dev_hp(cuda, "exact")
    h = hp.h
    step = h.last_i + 40 if step is None else step
    F = 2
    n = R * D
    assert n % 4 != 0 and (n > 2048 * 256 * 4) == (R > 5)
    rng = np.random.default_rng(R + D)
    w0 = (0.05 * rng.standard_normal((R, D))).astype(np.float32)
    m0 = (1e-3 * rng.standard_normal((R, D))).astype(np.float32)
    v0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e-6), size=(R, D))).astype(np.float32)
    idx = np.empty((B, F), dtype=np.int32)
    if R == 5:
        idx[:, 0], idx[:, 1] = (0, 2, 2, 0, 0, 2), (4, -1, 4, 4, -1, 4)                 # rows 1 and 3 are never looked up
    else:
        idx[:, 0], idx[:, 1] = rng.integers(0, 1000, size=B), R - 1 - rng.integers(0, 1000, size=B)
        idx[0, 1], idx[5, 0] = R - 1, -1
    uniq, seg, perm, cnt = _sort(cuda, lib, idx)
    rowgrad = (0.01 * rng.standard_normal((F, B, D))).astype(np.float32)
    un, cn = uniq.cpu().numpy(), cnt.cpu().numpy()
    g_in = np.zeros((R, D), dtype=np.float32)
    touched = np.zeros(R, dtype=bool)
    for f in range(F):
        for j in range(int(cn[f])):
            if un[f, j] >= 0:
                g_in[un[f, j]] = rowgrad[f, j]
                touched[un[f, j]] = True
    assert touched.sum() == len(np.unique(idx[idx >= 0])) and (R > 5 or not touched[[1, 3]].any()) and not touched.all()
    c = T.custom_case(h, w0, m0, v0, np.full(R, step - 1, dtype=np.int32), step, g_in=g_in)
    l2_only = T.replay_f64(w0[touched], m0[touched], v0[touched], step - 1, step, h)
    tab = Table(cuda, w0, m0, v0, np.zeros(R, dtype=np.int32))
    side = torch.full((F * B * 3 * D,), float("nan"), device=cuda)
    reg = torch.zeros(1, dtype=torch.float64, device=cuda)
    sd = _step(cuda, step)
    d_rg = _dev(cuda, rowgrad)
    call(lib, "cdc_embed_adam_touched", d_rg.data_ptr(), uniq.data_ptr(), cnt.data_ptr(), tab.w, tab.m, tab.v, side.data_ptr(), hp.c,
         sd.data_ptr(), B, F, D)
    call(lib, "cdc_embed_adam_dense_pass", tab.w, tab.m, tab.v, n, hp.c, sd.data_ptr(), reg.data_ptr())
    call(lib, "cdc_embed_adam_patch", side.data_ptr(), uniq.data_ptr(), cnt.data_ptr(), tab.w, tab.m, tab.v, B, F, D)
    got = tab.read(f"dense form R {R} D {D}")
    assert (got[3] == 0).all()                                                        # (the dense form has no last[])
    T.check(got[:3], c, T.K_EXACT, what=f"dense form R {R} D {D} step {step}")
    # the touched rows show the gradient step, not the L2-only step every other row takes
    b = T.bounds(c, T.K_EXACT)
    for q, i in (("w", 0), ("m", 1)):
        assert (np.abs(c.f64[i][touched] - l2_only[i]) > 4 * b[q][touched]).any(axis=1).all(), f"{q}: the two steps cannot be told apart"
    sq = np.square(w0.astype(np.float64))
    # two fp32 products and their fp32 sum per pair of weights, accumulated in double
    assert_bounded(reg.cpu().numpy(), np.array([sq.sum()]), sum_bound(np.array([sq.sum()]), 2, 1), "reg_sum: sum of w^2 before the step")
