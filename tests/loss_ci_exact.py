"""The contract of cdc_eval_loss_ci in float64 (helper of tests/test_eval_ci_cpu.py and tests/test_gpu_eval_ci.py; not a test).

Per segment of m rows the per-row term is cdc_eval_metrics': c = p for a positive, 1 - p for a negative, formed and clipped to
[eps32, 1 - eps32] in float32, l = -log(c) in double (math.log).  Then, with math.fsum (correctly rounded sums),

    loss = sum l / m        var = sum (l_i - loss)^2 / (m (m - 1))                  (a second, centred pass)

and with a second vector (terms k_i): loss_b, var_b, delta = loss - loss_b and var_delta = the formula of var on d_i = l_i - k_i,
centred on sum d / m.  Every figure is None for a segment without rows or with a single class.
"""
import math

import numpy as np

EPS32 = np.float32(1.1920928955078125e-07)                                  # numpy.finfo(float32).eps
HI32 = np.float32(1.0) - EPS32


def loss_terms(y, p):
    """-> list of the per-row terms (Python floats)"""
    p = np.asarray(p, dtype=np.float32)
    pos = np.asarray(y) != 0
    c = np.where(pos, p, np.float32(1.0) - p).astype(np.float32)            # float32 subtraction, as the kernel's
    c = np.where(c < EPS32, EPS32, np.where(c > HI32, HI32, c)).astype(np.float32)
    return [-math.log(float(v)) for v in c]


def centred(t):
    """-> (mean, sum of the centred squares / (m (m - 1))) of the values t, m >= 2"""
    m = len(t)
    mean = math.fsum(t) / m
    return mean, math.fsum((v - mean) ** 2 for v in t) / (m * (m - 1))


def loss_ci_rows(y, pa, pb=None):
    """One set of rows -> dict: rows, P, loss, var (and loss_b, var_b, delta, var_delta with pb), and the terms themselves under
    "terms" (and "terms_b") for the bounds of the device test."""
    y = np.asarray(y)
    m, P = len(y), int((y != 0).sum())
    keys = ("loss", "var") + (("loss_b", "var_b", "delta", "var_delta") if pb is not None else ())
    r = {"rows": m, "P": P, **{k: None for k in keys}}
    if m == 0 or P == 0 or P == m:
        return r
    la = loss_terms(y, pa)
    r["terms"] = la
    r["loss"], r["var"] = centred(la)
    if pb is not None:
        lb = loss_terms(y, pb)
        r["terms_b"] = lb
        r["loss_b"], r["var_b"] = centred(lb)
        r["delta"] = r["loss"] - r["loss_b"]
        r["var_delta"] = centred([a - b for a, b in zip(la, lb)])[1]
    return r


def loss_ci_exact(y, pa, pb=None, domain=None, n_domain=1):
    """Every figure of cdc_eval_loss_ci: a list with n_domain + 1 entries (domains 0..n_domain-1, then ALL rows) of
    loss_ci_rows' dicts."""
    y, pa = np.asarray(y), np.asarray(pa, dtype=np.float32)
    pb = None if pb is None else np.asarray(pb, dtype=np.float32)
    out = []
    for d in range(n_domain + 1):
        mk = np.ones(len(y), dtype=bool) if d == n_domain or domain is None else np.asarray(domain) == d
        out.append(loss_ci_rows(y[mk], pa[mk], None if pb is None else pb[mk]))
    return out


def as_float(v):
    return float("nan") if v is None else float(v)
