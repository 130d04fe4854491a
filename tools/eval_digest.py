"""Digest of the device evaluation calls, for comparing two builds of the library bit for bit.

    python tools/eval_digest.py              every public eval_* call on small fixed inputs (needs a GPU): per call one line with the
                                             workspace byte count, the error word and a SHA-256 of every returned tensor's bytes
    python tools/eval_digest.py --workspace  no device: the fixed workspace total every cdc_eval_* entry names when it refuses a
                                             workspace of 8 bytes, over a grid of sizes and options

Every figure of these calls is defined to be order-independent and bit-reproducible, so two runs, and two builds that compute the
same thing, print the same lines.  The library is whatever cdcmdr_amd loads: swap libcdcmdr.so and start a fresh process."""
import ctypes as C
import hashlib
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd import _lib as L          # noqa: E402
from cdcmdr_amd import evaluate as E      # noqa: E402

N_USER, N_ITEM, KS, N_REP = 37, 23, (1, 3), 9


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def flat(name, v, out):
    if v is None:
        out.append(f"{name}=None")
    elif torch.is_tensor(v):
        out.append(f"{name}={sha(v)}")
    else:                                                                  # a namedtuple
        for k in v._fields:
            flat(f"{name}.{k}" if name else k, getattr(v, k), out)


def inputs(n, n_domain, bad):
    g = torch.Generator().manual_seed(1000 * n + n_domain)
    r = lambda hi: torch.randint(0, hi, (n,), generator=g)                  # noqa: E731
    pred, pred_b = (r(17) / 16).float(), (r(17) / 16).float()               # sixteenths: tie runs cross chunk and slice bounds
    label, user, item = r(2).to(torch.int16), r(N_USER).to(torch.int32), r(N_ITEM).to(torch.int32)
    label[user < 3] = 0                                                    # users in one class only
    label[(user >= 3) & (user < 6)] = 1
    X = None
    if n_domain > 1:                                                       # a strided column view; domain 1 empty, the last single-class
        X = torch.stack([r(5), r(2) * (n_domain - 1), r(5)], dim=1).to(torch.int32)
        label[X[:, 1] == n_domain - 1] = 1
    if bad:                                                                # a NaN score, a domain of n_domain, a label of 2
        pred[n // 3] = float("nan")
        label[n - 1] = 2
        if X is not None:
            X[n // 2, 1] = n_domain
    dev = torch.device("cuda:0")
    X = None if X is None else X.to(dev)
    return dict(pred=pred.to(dev), pred_b=pred_b.to(dev), label=label.to(dev), user=user.to(dev), item=item.to(dev),
                domain=None if X is None else X[:, 1], weight=(torch.arange(N_USER, dtype=torch.float64) % 5 + 1).to(dev))


def cases(d, n, nd):
    """(tag, function, workspace bytes, thunk) of every call at one input"""
    lib = L.load()
    p, pb, y, u, dom, w = d["pred"], d["pred_b"], d["label"], d["user"], d["domain"], d["weight"]
    yield "metrics", E.eval_metrics, lib.cdc_eval_workspace_bytes(n, nd), lambda: E.eval_metrics(p, y, dom, nd)
    for wt in (None, w):
        yield f"gauc w={wt is not None}", E.eval_gauc, lib.cdc_eval_gauc_workspace_bytes(n, nd, N_USER), \
            lambda wt=wt: E.eval_gauc(p, y, u, N_USER, dom, nd, wt)
    yield "rank", E.eval_rank, lib.cdc_eval_rank_workspace_bytes(n, nd, N_USER, len(KS)), lambda: E.eval_rank(p, y, u, N_USER, dom, nd, KS, w)
    for it in (None, d["item"]):
        yield f"topk item={it is not None}", E.eval_topk, lib.cdc_eval_topk_workspace_bytes(n, nd, N_USER, int(it is not None)), \
            lambda it=it: topk_fields(E.eval_topk(p, u, N_USER, dom, nd, it, 3))
    for b in (None, pb):
        pr = int(b is not None)
        yield f"auc_ci paired={pr}", E.eval_auc_ci, lib.cdc_eval_auc_delong_workspace_bytes(n, nd, pr), lambda b=b: E.eval_auc_ci(p, y, dom, nd, b)
        yield f"loss_ci paired={pr}", E.eval_loss_ci, lib.cdc_eval_loss_ci_workspace_bytes(n, nd, pr), lambda b=b: E.eval_loss_ci(p, y, dom, nd, b)
        yield f"gauc_ci paired={pr}", E.eval_gauc_ci, lib.cdc_eval_gauc_ci_workspace_bytes(n, nd, N_USER, pr), \
            lambda b=b: E.eval_gauc_ci(p, y, u, N_USER, dom, nd, w, b)
        for cl in (None, u):
            gauc = int(cl is not None)
            yield f"bootstrap paired={pr} gauc={gauc}", E.eval_bootstrap, \
                lib.cdc_eval_bootstrap_workspace_bytes(n, nd, N_USER if gauc else 0, N_REP, gauc), \
                lambda b=b, cl=cl: E.eval_bootstrap(p, y, cl, N_USER if cl is not None else None, dom, nd, N_REP, 7, w, None, b)
        for rep in (0, N_REP):
            yield f"rank_ci paired={pr} n_rep={rep}", E.eval_rank_ci, lib.cdc_eval_rank_ci_workspace_bytes(n, nd, N_USER, len(KS), pr, rep), \
                lambda b=b, rep=rep: E.eval_rank_ci(p, y, u, N_USER, dom, nd, KS, w, b, rep, 7)
        for bins in (2, 10):
            yield f"calibration_bootstrap paired={pr} n_bins={bins}", E.eval_calibration_bootstrap, \
                lib.cdc_eval_calibration_bootstrap_workspace_bytes(n, nd, bins, N_REP, pr), \
                lambda b=b, bins=bins: E.eval_calibration_bootstrap(p, y, u, N_USER, dom, nd, bins, N_REP, 7, b)
    for bins in (2, 10):
        yield f"calibration n_bins={bins}", E.eval_calibration, lib.cdc_eval_calibration_workspace_bytes(n, nd, bins), \
            lambda bins=bins: E.eval_calibration(p, y, dom, nd, bins)
    yield "isotonic", E.eval_isotonic_fit, lib.cdc_eval_isotonic_fit_workspace_bytes(n, nd), lambda: isotonic_fields(p, y, dom, nd)
    for method in E.PLATT_METHODS:
        for inp in E.PLATT_INPUTS:
            x = p if inp == "prob" else (p - 0.5) * 8
            yield f"platt {method} {inp}", E.eval_platt_fit, lib.cdc_eval_platt_fit_workspace_bytes(n, nd), \
                lambda x=x, method=method, inp=inp: platt_fields(x, y, dom, nd, method, inp)


def topk_fields(t):
    return [f"{k}={sha(getattr(t, k))}" if getattr(t, k) is not None else f"{k}=None"
            for k in ("domain", "user", "start", "rows", "row", "score", "item", "n_out")]


def isotonic_fields(p, y, dom, nd):
    f = E.eval_isotonic_fit(p, y, dom, nd)
    nb = int(f.start[-1].item())                                           # the block tensors are written up to start[-1] only
    out = [f"start={sha(f.start)}", f"rows={sha(f.rows)}", f"seg_positives={sha(f.seg_positives)}"]
    out += [f"{k}={sha(getattr(f, k)[:nb])}" for k in ("x_lo", "x_hi", "count", "positives", "value")]
    if nb:
        out.append(f"apply={sha(E.eval_isotonic_apply(p, f, dom, nd, eps=1e-6))} apply_err={int(E.eval_isotonic_apply.last_err.item())}")
    return out


def platt_fields(x, y, dom, nd, method, inp):
    f = E.eval_platt_fit(x, y, dom, nd, method, inp)
    out = []
    flat("", f, out)
    out.append(f"apply={sha(E.eval_platt_apply(x, f, dom, nd, None, inp))} apply_err={int(E.eval_platt_apply.last_err.item())}")
    return out


def digest():
    for bad in (0, 1):
        for n in (1, 257, 5000):
            for nd in (1, 3):
                d = inputs(n, nd, bad)
                for tag, fn, nbytes, thunk in cases(d, n, nd):
                    r = thunk()
                    fields = r if isinstance(r, list) else []
                    if not isinstance(r, list):
                        if isinstance(r, tuple) and not hasattr(r, "_fields"):
                            for i, t in enumerate(r):
                                flat(str(i), t, fields)
                        else:
                            flat("", r, fields)
                    print(f"n={n} n_domain={nd} bad={bad} {tag}: ws={nbytes} err={int(fn.last_err.item())} " + " ".join(fields), flush=True)


def workspace():
    """every entry with good arguments and a workspace of 8 bytes: the refusal names the fixed total"""
    lib = L.load()
    p, q = C.c_void_p(4096), None                                          # non-null and aligned, never dereferenced; q: an absent vector

    def ask(tag, rc):
        m = re.search(rb"workspace 8 < (\d+) bytes", lib.cdc_last_error())
        print(f"{tag}: rc={rc} fixed={m.group(1).decode() if m else repr(lib.cdc_last_error())}")

    for n in (1, 257, 5000, 500000):
        for nd in (1, 3, 50):
            at = f"n={n} n_domain={nd}"
            ask(f"{at} eval_metrics", lib.cdc_eval_metrics(p, p, p, 1, n, nd, p, p, None, p, 8, None))
            ask(f"{at} eval_gauc", lib.cdc_eval_gauc(p, p, p, 1, N_USER, p, 1, nd, None, n, p, p, None, p, 8, None))
            ask(f"{at} eval_isotonic_fit", lib.cdc_eval_isotonic_fit(p, p, p, 1, n, nd, p, p, p, p, p, p, 2 * n, p, p, None, p, 8, None))
            ask(f"{at} eval_platt_fit", lib.cdc_eval_platt_fit(p, p, p, 1, n, nd, 0, 0, 1e-7, 1e-10, 32, p, p, p, p, p, p, p, p, p, None, p, 8, None))
            for item in (q, p):
                ask(f"{at} eval_topk item={int(item is not None)}",
                    lib.cdc_eval_topk(p, p, 1, N_USER, p, 1, nd, item, 1, 3, n, p, p, p, p, p, p, p, None, p, 8, None))
            for n_k in (1, 3):
                ask(f"{at} eval_rank n_k={n_k}", lib.cdc_eval_rank(p, p, p, 1, N_USER, p, 1, nd, None, p, n_k, p, n, p, p, None, p, 8, None))
            for bins in (2, 10):
                ask(f"{at} eval_calibration n_bins={bins}", lib.cdc_eval_calibration(p, p, p, 1, n, nd, bins, p, p, p, p, p, None, p, 8, None))
            for b in (q, p):
                pr = int(b is not None)
                ask(f"{at} eval_auc_delong paired={pr}", lib.cdc_eval_auc_delong(p, b, p, p, 1, n, nd, p, p, None, p, 8, None))
                ask(f"{at} eval_loss_ci paired={pr}", lib.cdc_eval_loss_ci(p, b, p, p, 1, n, nd, p, p, None, p, 8, None))
                ask(f"{at} eval_gauc_ci paired={pr}", lib.cdc_eval_gauc_ci(p, b, p, p, 1, N_USER, p, 1, nd, None, n, p, p, None, p, 8, None))
                for rep in (9, 200):
                    for gauc in (0, 1):
                        ask(f"{at} eval_bootstrap paired={pr} n_rep={rep} gauc={gauc}",
                            lib.cdc_eval_bootstrap(p, b, p, p, 1, N_USER, p, 1, nd, None, n, rep, 7, gauc, p, p, None, p, 8, None))
                    for bins in (2, 10):
                        ask(f"{at} eval_calibration_bootstrap paired={pr} n_rep={rep} n_bins={bins}",
                            lib.cdc_eval_calibration_bootstrap(p, b, p, p, 1, N_USER, p, 1, nd, bins, n, rep, 7, p, p, None, p, 8, None))
                for rep in (0, 9, 200):
                    for n_k in (1, 3):
                        ask(f"{at} eval_rank_ci paired={pr} n_rep={rep} n_k={n_k}",
                            lib.cdc_eval_rank_ci(p, b, p, p, 1, N_USER, p, 1, nd, None, p, n_k, p, n, rep, 7, p, p if rep else None, p,
                                                 p if rep else None, None, p, 8, None))


if __name__ == "__main__":
    workspace() if "--workspace" in sys.argv[1:] else digest()
