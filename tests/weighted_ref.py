"""float64 references of the WEIGHTED fused loss for the GPU tests of the fused launches (tests/test_gpu_weighted_fused.py), held on
the CPU by tests/test_weighted_loss_cpu.py.  No GPU.

The weighted loss is torch's F.binary_cross_entropy(p, y, weight=w, reduction='mean'): row b's loss term and its gradient times
w[b], the mean still over the batch's rows.  On the device the weight is one more fp32 factor of the finished unweighted gradient
and one exact product in double for the loss term, so every bound of the unweighted references holds with its row terms scaled by
w and one rounding more.

Towers: tower_ref.ref_backward takes its logit gradients from tower_ref.logit_gradients, which it looks up at call time;
`tower_logit_gradients(w)` wraps that function, and a test puts the wrapper in its place with monkeypatch.setattr(tower_ref,
"logit_gradients", ...).  tests/tower_ref.py itself stays as it is.
Head and row-dot: `head_backward` restates tests/test_gpu_head.py's ref_backward for the fused-BCE form with weights (plain stores,
no NULL output), with that file's counts: cd = 7 + 3 roundings of d, one more for the weight."""
import numpy as np

import tower_ref as R
from helpers import OUT_FIG, SUM_FIG, U24, capped, sum_bound, ulp32

f64 = lambda a: np.asarray(a, dtype=np.float64)
_tower_logit_gradients = R.logit_gradients      # the unweighted function, whatever a test puts in its place later


def weights(name, M):
    """seeded by the case's name: uniform [0, 3), every eighth exactly 0, one 2^-20 and one 1024"""
    rng = np.random.default_rng(sum((i + 3) * ord(ch) for i, ch in enumerate(name)) + M)
    w = rng.uniform(0.0, 3.0, size=M).astype(np.float32)
    w[7::8] = 0.0
    w[M - 1] = 1024.0
    if M >= 2:
        w[M - 2] = 2.0 ** -20
    return w


def tower_logit_gradients(w):
    """tower_ref.logit_gradients with row weights: d, the loss rows and their magnitudes times w, one rounding more on d"""
    wd = f64(w)

    def fn(c, D, out, defect=None):
        d, cd, loss = _tower_logit_gradients(c, D, out, defect)
        assert R.bce(c) and defect is None and wd.shape == (c["M"],)
        M = c["M"]
        o, y = f64(out)[np.arange(M), R.own_tower(c, D)], f64(D["y"])
        with np.errstate(divide="ignore", invalid="ignore"):
            la, lb = np.maximum(np.log1p(-o), -100.0), np.maximum(np.log(o), -100.0)
        rows, mag = (y - 1.0) * la - y * lb, np.abs((y - 1.0) * la) + np.abs(y * lb)
        inv = R.inv_count(c)
        total = float(np.sum(wd * rows) * inv)
        bound = inv * np.sum(wd * (4 * R.LOSS_ULPS_HOST * ulp32(mag)) + U24 * wd * mag) + 2 * U24 * abs(total)
        return d * wd[:, None], cd + 1, (np.array([total]), capped(np.array([bound]), total, OUT_FIG), loss[2])
    return fn


HEAD_LOSS_ULPS_HOST = 2.4                       # tests/test_gpu_head.py ref_backward


def head_backward(K, wide_K, n_add, D, out32, w, inv):
    """The fused-BCE backward of cdc_head_args / cdc_rowdot_bwd_args with row weights as name -> (want, bound): towers of widths K,
    an optional wide term, n_add addends, every gradient a plain store.  D: x, w (lists), wx, ww, wb, y, group as
    tests/test_gpu_head.py's make_data gives them.  The names are that file's.  w = None: the unweighted launch (the NULL pointer),
    without the weight's rounding."""
    M, nt = out32.shape[0], len(K)
    o, wd, y = f64(out32), (np.ones(M) if w is None else f64(w)), f64(D["y"])
    own = np.zeros(M, dtype=np.int64) if D["group"] is None else D["group"].copy()
    own[(own < 0) | (own >= nt)] = 0
    oo = o[np.arange(M), own]
    with np.errstate(divide="ignore"):
        la, lb = np.maximum(np.log1p(-oo), -100.0), np.maximum(np.log(oo), -100.0)
    rows, mag = (y - 1.0) * la - y * lb, np.abs((y - 1.0) * la) + np.abs(y * lb)
    loss = float(np.sum(wd * rows) * inv)
    b_loss = inv * np.sum(wd * (4 * HEAD_LOSS_ULPS_HOST * ulp32(mag)) + U24 * wd * mag) + 2 * U24 * abs(loss)
    Rr = {"loss": (np.array([loss]), capped(np.array([b_loss]), loss, OUT_FIG))}
    dout = np.zeros((M, nt))
    dout[np.arange(M), own] = inv * (oo - y) / np.maximum((1.0 - oo) * oo, 1e-12) * wd
    cd = 7 + (0 if w is None else 1) + 3        # the unweighted dout, the weight, dout o (1 - o)
    d = dout * o * (1.0 - o)
    ad = np.abs(d)
    dsum, a_dsum = d.sum(1), ad.sum(1)
    for t, Kt in enumerate(K):
        x, wt = f64(D["x"][t]), f64(D["w"][t])
        v = d[:, t:t + 1] * wt[None, :]
        Rr[f"dx{t}"] = (v, capped((cd + 1) * U24 * np.abs(v), v, OUT_FIG))
        Rr[f"dw{t}"] = ((d[:, t] @ x).reshape(1, Kt), capped(sum_bound(ad[:, t] @ np.abs(x), M, cd + 1), d[:, t] @ x, SUM_FIG).reshape(1, Kt))
        Rr[f"dbias{t}"] = (np.array([[d[:, t].sum()]]), capped(sum_bound(ad[:, t].sum(), M, cd), d[:, t].sum(), SUM_FIG).reshape(1, 1))
    for i in range(n_add):
        Rr[f"d_addend{i}"] = (dsum.reshape(M, 1), capped(sum_bound(a_dsum, nt, cd), dsum, OUT_FIG).reshape(M, 1))
    if wide_K:
        wx, ww = f64(D["wx"]), f64(D["ww"])
        v = dsum[:, None] * ww[None, :]
        Rr["wide_dx"] = (v, capped(sum_bound(a_dsum[:, None] * np.abs(ww)[None, :], nt, cd + 1), v, OUT_FIG))
        Rr["wide_dw"] = ((dsum @ wx).reshape(1, wide_K), capped(sum_bound(a_dsum @ np.abs(wx), M + nt, cd + 1), dsum @ wx, SUM_FIG).reshape(1, wide_K))
        if D.get("wb") is not None:
            Rr["wide_dbias"] = (np.array([[dsum.sum()]]), capped(sum_bound(a_dsum.sum(), M + nt, cd), dsum.sum(), SUM_FIG).reshape(1, 1))
    return Rr
