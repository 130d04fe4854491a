"""Platt / temperature / bias scaling restated in float64 numpy: the contract of cdc_eval_platt_fit / cdc_eval_platt_apply
(include/cdcmdr.h) as plain sequential code — the logit-scale score z, Platt's smoothed targets, the objective
F(a, b) = sum t softplus(-u) + (1 - t) softplus(u), u = a z + b, and its minimiser by Newton steps with a backtracking line search run
to a mean gradient <= 1e-13.  The device stops at 1e-10, so this is the better answer of the two; tests/test_platt_cpu.py holds it to
closed forms and to sklearn's LogisticRegression."""
import numpy as np

CONVERGED, EMPTY, SLOPE_FIXED = 1, 2, 4
METHODS = ("platt", "temperature", "bias")
REF_GTOL = 1e-13
MAX_STEPS = 32                       # the device's default cap: the reference must stay inside it on every test input
STATS = {"steps": 0, "evals": 0}     # the largest counts over all fits made so far


def platt_z(score, input="prob", clip=1e-7):
    """float32 scores -> float64 z, clamped to +-log((1 - clip) / clip); a bad score (NaN, or a probability outside [0, 1]) gives NaN"""
    x = np.asarray(score, np.float32).astype(np.float64)
    Z = np.log((1.0 - clip) / clip)
    with np.errstate(divide="ignore", invalid="ignore"):
        if input == "prob":
            z = np.where((x >= 0) & (x <= 1), np.log(x) - np.log1p(-x), np.nan)
        else:
            assert input == "logit"
            z = x.copy()
    return np.where(np.isnan(z), np.nan, np.clip(z, -Z, Z))


def targets(y):
    y = np.asarray(y).astype(bool)
    P = int(y.sum())
    N = y.size - P
    return np.where(y, (P + 1.0) / (P + 2.0), 1.0 / (N + 2.0))


def softplus(u):
    return np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))


def sigmoid(u):
    e = np.exp(-np.abs(u))
    return np.where(u >= 0, 1.0, e) / (1.0 + e)


def objective(z, t, a, b):
    """-> (F, gradient [2], Hessian [2, 2]) as SUMS over the rows"""
    u = a * z + b
    p = sigmoid(u)
    r, w = p - t, p * (1.0 - p)
    F = float(np.sum(softplus(u) - t * u))
    g = np.array([np.sum(r * z), np.sum(r)])
    H = np.array([[np.sum(w * z * z), np.sum(w * z)], [np.sum(w * z), np.sum(w)]])
    return F, g, H


def mean_gradient(z, y, a, b, free):
    """inf-norm over the free parameters of the mean gradient of F at (a, b)"""
    z = np.asarray(z, np.float64)
    _, g, _ = objective(z, targets(y), a, b)
    return float(np.max(np.abs(g[list(free)])) / z.size)


def bce(z, y, a, b):
    """plain mean cross-entropy of sigmoid(a z + b) against the 0/1 labels"""
    u = a * np.asarray(z, np.float64) + b
    return float(np.mean(softplus(u) - np.asarray(y).astype(np.float64) * u))


def free_parameters(z, method):
    """-> (indices of the free parameters among (a, b), status bits)"""
    if method == "temperature":
        return (0,), 0
    if method == "bias":
        return (1,), 0
    assert method == "platt"
    if np.min(z) == np.max(z):
        return (1,), SLOPE_FIXED
    return (0, 1), 0


def fit_rows(z, y, method="platt", gtol=REF_GTOL):
    """One segment's rows -> (a, b, mean Hessian [2, 2] at the optimum, status, free parameters).  Asserts its own convergence
    inside MAX_STEPS Newton steps."""
    z = np.asarray(z, np.float64)
    m = z.size
    assert m > 0 and not np.isnan(z).any()
    t = targets(y)
    free, status = free_parameters(z, method)
    idx = np.array(free)
    th = np.array([1.0, 0.0])
    F, g, H = objective(z, t, *th)
    steps, evals = 0, 1
    while np.max(np.abs(g[idx])) / m > gtol:
        assert steps < MAX_STEPS, ("the reference did not converge", method, m, np.max(np.abs(g[idx])) / m)
        d = np.zeros(2)
        d[idx] = -np.linalg.solve(H[np.ix_(idx, idx)], g[idx])
        gd, lam = float(g @ d), 1.0
        while True:
            F1, g1, H1 = objective(z, t, *(th + lam * d))
            evals += 1
            if F1 <= F + 1e-4 * lam * gd + 1e-12 * abs(F):
                break
            lam *= 0.5
            assert lam > 2.0 ** -40, ("the line search of the reference failed", method, m)
        th, F, g, H = th + lam * d, F1, g1, H1
        steps += 1
    STATS["steps"], STATS["evals"] = max(STATS["steps"], steps), max(STATS["evals"], evals)
    return float(th[0]), float(th[1]), H / m, status | CONVERGED, free


def inv_norm(Hbar, free):
    """inf-norm of the inverse of the mean Hessian over the free parameters"""
    idx = np.array(free)
    return float(np.max(np.sum(np.abs(np.linalg.inv(Hbar[np.ix_(idx, idx)])), axis=1)))


def platt_exact(y, score, dom=None, n_domain=1, method="platt", input="prob", clip=1e-7):
    """-> per segment (domains 0..n_domain-1, then ALL rows) a dict(a, b, H, status, free, rows, positives, loss_before, loss_after),
    for an empty segment dict(a=1, b=0, status=EMPTY, rows=0, positives=0)"""
    y = np.asarray(y).astype(np.int64)
    z = platt_z(score, input, clip)
    dom = np.zeros(len(y), np.int64) if dom is None else np.asarray(dom)
    out = []
    for s in range(n_domain + 1):
        sel = np.ones(len(y), bool) if s == n_domain else dom == s
        if not sel.any():
            out.append(dict(a=1.0, b=0.0, status=EMPTY, rows=0, positives=0))
            continue
        a, b, H, status, free = fit_rows(z[sel], y[sel], method)
        out.append(dict(a=a, b=b, H=H, status=status, free=free, rows=int(sel.sum()), positives=int(y[sel].sum()),
                        loss_before=bce(z[sel], y[sel], 1.0, 0.0), loss_after=bce(z[sel], y[sel], a, b), z=z[sel], y=y[sel]))
    return out


def platt_apply(score, a, b, input="prob", clip=1e-7, eps=0.0):
    """float32 map values: (float32)(1 / (1 + exp(-(a z + b)))), a and b scalars or one entry per row; a bad score gives NaN"""
    z = platt_z(score, input, clip)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (1.0 / (1.0 + np.exp(-(np.asarray(a, np.float64) * z + np.asarray(b, np.float64))))).astype(np.float32)
    if eps > 0:
        e = np.float32(eps)
        out = np.where(np.isnan(out), out, np.clip(out, e, np.float32(1) - e))
    return out


KINDS = ("calibrated", "odds x10", "slope 0.4 shift -1")


def ctr_like(rng, n, kind, input="prob"):
    """-> (score float32, label int16).  A row's true logit q ~ N(-3, 1.5^2), its label ~ Bernoulli(sigmoid(q)); the model's logit is
    q ("calibrated"), q + log 10 ("odds x10": trained on negatives down-sampled tenfold; the repair is b = -log 10) or (q + 1) / 0.4
    (over-confident: the repair is a = 0.4, b = -1); a tenth of the rows share one score."""
    q = rng.normal(-3.0, 1.5, n)
    q = np.where(rng.random(n) < 0.1, q[0], q)
    y = (rng.random(n) < sigmoid(q)).astype(np.int16)
    model = {"calibrated": q, "odds x10": q + np.log(10.0), "slope 0.4 shift -1": (q + 1.0) / 0.4}[kind]
    return (sigmoid(model) if input == "prob" else model).astype(np.float32), y
