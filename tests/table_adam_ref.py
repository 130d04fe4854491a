"""References for the lazy table's Adam replay (helper of tests/test_table_adam_cpu.py and tests/test_gpu_table_adam.py; not a test).

A table row's (w, m, v) are valid for step last[row]; the kernels replay the L2-only Adam steps last+1 .. target on demand
(csrc/common.h adam_replay_wave and its scaled fast form, csrc/embedding.hip's flush and catch-up launches).  Three restatements
of that replay, none of which runs a kernel:

  replay_f64              the recurrence of adam_elem() with g_in = 0 in float64, from the fp32 constants and the fp32 step-scalar
                          table the kernels read (clamped at its last row)
  replay_c32              the same loop through oracle/adam_elem_ref.c: fp32, operation for operation the device's exact routine
  replay_scaled_emulated  an fp32 numpy emulation of adam_scaled_step_pk with the in/out scaling of adam_replay_wave_scaled and the
                          host-built table of optim.replay_constants; optionally with every sqrt and reciprocal perturbed by a random
                          -1/0/+1 ulp (the stated accuracy of the hardware instructions), and with seeded DEFECTS

The yardstick of every comparison is E_ref, the deviation of the fp32 restatement from float64 on the case's own elements: a path
under test may deviate from float64 by K * E_ref + floor (bounds()).  K_EXACT = 4 for the exact path (the arithmetic is the
restatement's own; the one known difference is the last bit of the update quotient in ~0.2 % of element-steps).  K_FAST is
MEASURED, from references only, by tests/test_table_adam_cpu.py: the emulation with the +-1-ulp perturbation over the whole case
matrix below (every (wd, l2) of the scaled modes x TARGETS x STATES, 192 rows, 256 or 32 columns), worst raw ratio
max|emulated - f64| / E_ref per quantity:

      w 2.57      m 3.08      v 2.72        (34 cases; the test prints the figures and where they occur, run it with -s)

K_FAST is twice the worst ratio rounded up to a power of two — the factor two is headroom for accumulation orders the emulation
does not sample — so K_FAST = 8 for each of the three; the CPU test asserts that the emulation stays under K_FAST / 2 and that every seeded
defect exceeds the fast bound in at least one case.
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K_EXACT = {"w": 4.0, "m": 4.0, "v": 4.0}
K_FAST = {"w": 8.0, "m": 8.0, "v": 8.0}
DEFECTS = ("short", "long", "shift", "no_wd", "c2_zero")

# the modes of the matrix: name -> (fast_replay, weight_decay, table l2)
MODES = {"exact": (0, 1e-8, 1e-5), "scaled": (1, 1e-8, 1e-5), "scaled_l2_0": (1, 1e-8, 0.0), "unscaled": (1, 0.0, 0.0)}
STATES = ("fresh", "trained", "big")
ROWS, COLS_SHALLOW, COLS_DEEP, SHALLOW = 192, 256, 32, 64


def f32(x):
    return float(np.float32(x))


class HP:
    """The hyper-parameters as the kernels get them (optim.FusedAdam._hp): fp32 values held in Python floats, the truncated
    step-scalar table and what optim.replay_constants builds from it."""

    def __init__(self, wd=1e-8, l2=1e-5, lr=1e-3, betas=(0.9, 0.99), eps=1e-8):
        from cdcmdr_amd.optim import replay_constants, step_scalar_table
        self.lerp_w, self.beta2, self.omb2, self.eps, self.wd = f32(1.0 - betas[0]), f32(betas[1]), f32(1.0 - betas[1]), f32(eps), f32(wd)
        self.l2 = l2
        self.l2_twice = 2.0 * f32(l2)
        self.tab_t = step_scalar_table(lr, betas[0], betas[1], n=65536, truncate=True)
        self.tab = self.tab_t.numpy()
        self.last_i = self.tab.shape[0] - 1
        self.rc = replay_constants(self.tab_t, self.lerp_w, self.omb2, self.eps, self.wd, l2)

    def scalars(self, s):
        i = min(max(int(s), 0), self.last_i)                       # step_scalars_at / the replay loops: clamped at the last row
        return self.tab[i, 0], self.tab[i, 1]


@functools.lru_cache(maxsize=None)
def hp_of(wd, l2):
    return HP(wd=wd, l2=l2)


def _rows(frm, shape):
    frm = np.asarray(frm, dtype=np.int64)
    return np.broadcast_to(frm.reshape(-1, *([1] * (len(shape) - 1))), shape) if frm.ndim else np.full(shape, int(frm))


def replay_f64(w, m, v, frm, to, hp, g_in=None):
    """-> float64 (w, m, v) after the steps frm < s <= to of adam_elem (g_in: a batch gradient added at EVERY replayed step —
    used for a single step of the dense form; None = the L2-only recurrence).  frm: scalar or one value per row.  Rows are
    grouped by their start step, so a table with a few deep rows costs what those rows cost."""
    out = [np.array(a, dtype=np.float64) for a in (w, m, v)]
    frm = _rows(frm, out[0].shape)
    g_all = np.zeros(out[0].shape) if g_in is None else np.array(g_in, dtype=np.float64)
    for f0 in np.unique(frm):
        if f0 >= to:
            continue
        sel = frm == f0
        w1, m1, v1, g0 = (x[sel] for x in (*out, g_all))
        for s in range(int(f0) + 1, int(to) + 1):
            ss, bc = (float(x) for x in hp.scalars(s))
            g = g0 + hp.l2_twice * w1
            g = g + w1 * hp.wd
            m1 = m1 + hp.lerp_w * (g - m1)
            v1 = v1 * hp.beta2 + (hp.omb2 * g) * g
            w1 = w1 + (-ss * m1) / (np.sqrt(v1) / bc + hp.eps)
        for x, y in zip(out, (w1, m1, v1)):
            x[sel] = y
    return tuple(out)


def replay_c32(w, m, v, frm, to, hp, g_in=None):
    """The same loop in fp32 through oracle/adam_elem_ref.c (rows grouped by their start step)."""
    from test_host_logic import _build_adam_ref
    lib = _build_adam_ref()
    out = [np.array(a, dtype=np.float32) for a in (w, m, v)]
    frm = _rows(frm, out[0].shape)
    g_all = np.zeros(out[0].shape, np.float32) if g_in is None else np.asarray(g_in, dtype=np.float32)
    for f0 in np.unique(frm):
        if f0 >= to:
            continue
        sel = frm == f0
        a, b, c, g = (np.ascontiguousarray(x[sel]) for x in (*out, g_all))
        for s in range(int(f0) + 1, int(to) + 1):
            ss, bc = hp.scalars(s)
            lib.adam_elem_ref(a.ctypes.data, b.ctypes.data, c.ctypes.data, g.ctypes.data, a.size, hp.lerp_w, hp.beta2, hp.omb2, hp.eps,
                              hp.wd, hp.l2_twice, float(ss), float(bc))
        for x, y in zip(out, (a, b, c)):
            x[sel] = y
    return tuple(out)


def _fma(a, b, c):
    """fp32 fma as the float64 product (exact) plus addend, rounded to fp32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _ulp_step(x, rng):
    """x moved by a random -1/0/+1 ulp (finite non-zero values only)"""
    if rng is None:
        return x
    bits = x.view(np.int32) + rng.integers(-1, 2, size=x.shape).astype(np.int32)
    y = bits.view(np.float32)
    return np.where(np.isfinite(x) & (x != 0) & np.isfinite(y), y, x).astype(np.float32)


def replay_scaled_emulated(w, m, v, frm, to, hp, rng=None, defect=None):
    """adam_replay_wave_scaled in numpy fp32: state scaled in by ik1 / ik2, adam_scaled_step_pk per step with the host table
    (C1, C2), scaled out by k + k_lo; rows with frm >= to come back untouched.  rng: perturb every sqrt and reciprocal by a random
    -1/0/+1 ulp.  defect: one of DEFECTS — 'short' / 'long' one step too few / too many, 'shift' the table read at s + 1, 'no_wd'
    the constants built without the weight-decay term, 'c2_zero' C2 (the eps term) forced to 0.  -> None if the defect does not
    exist for these hyper-parameters (no_wd with l2 = 0 leaves no scaled form at all)."""
    assert defect is None or defect in DEFECTS
    rc = hp.rc
    if defect == "no_wd":
        from cdcmdr_amd.optim import replay_constants
        rc = replay_constants(hp.tab_t, hp.lerp_w, hp.omb2, hp.eps, 0.0, hp.l2)
    if rc.replay_tab is None:
        assert defect == "no_wd", "no scaled form for these hyper-parameters"
        return None
    rt = rc.replay_tab.numpy()
    w0, m0, v0 = (np.array(a, dtype=np.float32) for a in (w, m, v))
    frm = _rows(frm, w0.shape)
    beta1, beta2 = np.float32(1.0) - np.float32(hp.lerp_w), np.float32(hp.beta2)
    W, M, V = w0.copy(), m0 * np.float32(rc.ik1), v0 * np.float32(rc.ik2)
    end = int(to) + {"short": -1, "long": 1}.get(defect, 0)
    for s in range(int(frm.min()) + 1, end + 1):
        i = min(s + (1 if defect == "shift" else 0), hp.last_i)
        C1, C2 = rt[i, 0], (np.float32(0.0) if defect == "c2_zero" else rt[i, 1])
        Mn = _fma(beta1, M, W)
        Vn = _fma(beta2, V, W * W)
        sq = _ulp_step(np.sqrt(Vn), rng)
        with np.errstate(divide="ignore"):
            r = _ulp_step(np.float32(1.0) / _fma(sq, C1, C2), rng)
        Wn = _fma(Mn, r, W)
        act = frm < s
        W, M, V = np.where(act, Wn, W), np.where(act, Mn, M), np.where(act, Vn, V)
    mo = _fma(M, np.float32(rc.k1), M * np.float32(rc.k1_lo))
    vo = _fma(V, np.float32(rc.k2), V * np.float32(rc.k2_lo))
    done = frm < to
    return np.where(done, W, w0), np.where(done, mo, m0), np.where(done, vo, v0)


# ----------------------------------------------------------------------------------------------------------------------
# the case matrix of the replay tests: (mode, target, state) -> a table of ROWS rows with mixed `last`
# ----------------------------------------------------------------------------------------------------------------------
def targets(hp):
    return (1, 8, 64, hp.last_i - 1, hp.last_i, hp.last_i + 1, hp.last_i + 300)


def matrix(mode):
    """(target, state) of a mode: `fresh` for the shallow targets only"""
    hp = hp_of(*MODES[mode][1:])
    return [(t, s) for t in targets(hp) for s in STATES if not (s == "fresh" and t > SHALLOW)]


Case = collections.namedtuple("Case", "mode target state hp w0 m0 v0 last f64 c32")


def case(mode, target, state):
    """The inputs and both references of one case.  Deep targets have COLS_DEEP columns, shallow ones COLS_SHALLOW; a test at
    emb_dim D uses the first D columns.  `last` mixes {0, 1, 3, target-1, target, target+1, a mid value} inside every wave."""
    return _case(MODES[mode][1], MODES[mode][2], target, state)._replace(mode=mode)


@functools.lru_cache(maxsize=None)
def _case(wd, l2, target, state):
    """(the exact and the scaled mode share hyper-parameters, hence data and references)"""
    mode = None
    hp = hp_of(wd, l2)
    cols = COLS_SHALLOW if target <= SHALLOW else COLS_DEEP
    rng = np.random.default_rng([int(round(wd * 1e9)), int(round(l2 * 1e9)), target, STATES.index(state)])
    w0 = (rng.standard_normal((ROWS, cols)) * (1.0 if state == "big" else 0.01)).astype(np.float32)
    if state == "fresh":
        m0, v0 = np.zeros((ROWS, cols), np.float32), np.zeros((ROWS, cols), np.float32)
    else:
        m0 = (1e-3 * rng.standard_normal((ROWS, cols))).astype(np.float32)
        v0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e-6), size=(ROWS, cols))).astype(np.float32)
    choice = np.array([0, 1, 3, target - 1, target, target + 1, max(target // 2, 0)], dtype=np.int32)
    last = np.maximum(choice[rng.integers(0, len(choice), size=ROWS)], 0).astype(np.int32)
    last[:len(choice)] = np.maximum(choice, 0)                       # every value occurs
    f64 = replay_f64(w0, m0, v0, last, target, hp)
    c32 = replay_c32(w0, m0, v0, last, target, hp)
    for a in (w0, m0, v0, last, *f64, *c32):
        a.setflags(write=False)
    return Case(mode, target, state, hp, w0, m0, v0, last, f64, c32)


def custom_case(hp, w0, m0, v0, frm, target, g_in=None):
    """a Case from the caller's own table: frm per row (a row the call must not touch: frm = target)"""
    frm = np.asarray(frm, dtype=np.int32)
    return Case(None, target, None, hp, w0, m0, v0, frm, replay_f64(w0, m0, v0, frm, target, hp, g_in),
                replay_c32(w0, m0, v0, frm, target, hp, g_in))


def ulp32_at(x):
    return float(np.spacing(np.float32(np.max(np.abs(x)))))


def errors(got, f64):
    """-> {w, m: |got - f64| per element; v: the same relative to the float64 value (absolute where that is 0)}"""
    e = {q: np.abs(np.asarray(g, dtype=np.float64) - r) for q, g, r in zip("wmv", got, f64)}
    with np.errstate(divide="ignore", invalid="ignore"):
        e["v"] = np.where(f64[2] != 0, e["v"] / np.abs(f64[2]), e["v"])
    return e


def e_ref(c, cols=None):
    """E_ref per quantity over the case's elements (the first `cols` columns)"""
    sl = slice(None) if cols is None else slice(0, cols)
    e = errors([a[:, sl] for a in c.c32], [a[:, sl] for a in c.f64])
    return {q: float(e[q].max()) for q in "wmv"}


def bounds(c, K, cols=None):
    """Allowed |got - f64| per element of w, m, v for the path with margin K (K_EXACT / K_FAST): K * E_ref + floor.  Floor: 2 ulp32
    at the case's largest reference magnitude for w and m; for v 2^-22 relative plus 1e-30 absolute, so that a value in the fp32
    subnormal range never decides a test."""
    sl = slice(None) if cols is None else slice(0, cols)
    E = e_ref(c, cols)
    f = [a[:, sl] for a in c.f64]
    return {"w": np.full(f[0].shape, K["w"] * E["w"] + 2 * ulp32_at(f[0])),
            "m": np.full(f[1].shape, K["m"] * E["m"] + 2 * ulp32_at(f[1])),
            "v": (K["v"] * E["v"] + 2.0 ** -22) * np.abs(f[2]) + 1e-30}


def ratios(got, c, cols=None):
    """worst raw ratio of |got - f64| to E_ref per quantity (v relative)"""
    sl = slice(None) if cols is None else slice(0, cols)
    f = [a[:, sl] for a in c.f64]
    e, E = errors(got, f), e_ref(c, cols)
    out = {}
    for q in "wmv":
        worst = float(e[q].max())
        out[q] = worst / E[q] if E[q] > 0 else (0.0 if worst == 0 else float("inf"))
    return out


def check(got, c, K, cols=None, what=""):
    """asserts got = (w, m, v) against float64 under bounds(); -> ratios"""
    sl = slice(None) if cols is None else slice(0, cols)
    f = [a[:, sl] for a in c.f64]
    b = bounds(c, K, cols)
    for q, g, r in zip("wmv", got, f):
        err = np.abs(np.asarray(g, dtype=np.float64) - r)
        bad = ~(err <= b[q])
        if bad.any():
            i = int(np.argmax(np.where(np.isnan(err), np.inf, err / b[q])))
            raise AssertionError(f"{what} {q}: {int(bad.sum())}/{err.size} off; worst |d|={err.flat[i]:.3e} allowed {b[q].flat[i]:.3e} "
                                 f"got {np.asarray(g).flat[i]:.9e} want {r.flat[i]:.9e} (row {i // err.shape[1]}, last {c.last[i // err.shape[1]]}, "
                                 f"E_ref {e_ref(c, cols)[q]:.3e})")
    return ratios(got, c, cols)
