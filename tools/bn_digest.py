"""Digest of the BatchNorm launches (cdc_bn_fwd, cdc_bn_bwd), for comparing two builds of the library bit for bit.

    python tools/bn_digest.py      every spec of tests/bn_ref.py (geometry, row groups, flags) forward and backward, and every
                                   data-parallel split through phases 1 and 2 (needs a GPU): per case one line with a SHA-256 of
                                   every returned array — y, yh, the saved and running statistics, num_batches_tracked, dx, dxh,
                                   dgamma, dbeta, and the exchange buffers after phase 1

The launches sum in a fixed order, so two runs, and two builds that compute the same thing, print the same lines; the float64
margins of tests/test_gpu_batchnorm.py would let another summation order pass, this listing does not.  The buffers and argument
blocks are the tests' own (Launch).  The library is whatever cdcmdr_amd loads: swap libcdcmdr.so and start a fresh process."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bn_ref as R                      # noqa: E402
import test_gpu_batchnorm as T          # noqa: E402


def sha(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]


def fields(got):
    """the arrays of fwd_read / bwd_read, segment by segment"""
    return " ".join(f"{k}{i}={sha(np.asarray(v))}" for i, g in enumerate(got) for k, v in g.items())


def single(dev, s):
    D = R.make_data(s)
    la = T.Launch(dev, s, D)
    got = la.forward()
    back = la.backward(*T.saved_from(s, D, got))
    print(f"{s['name']} M={s['M']} {R.family(s)}: {fields(got)} | {fields(back)}", flush=True)


def data_parallel(dev, name, pad):
    """the two ranks of tests/test_gpu_batchnorm.py::test_bn_data_parallel_phases on one device"""
    u, ranks, parts = R.dp_specs(name, pad)
    Du = R.make_data(u)
    n_ex = 2 * sum(u["C"]) + len(u["C"])
    las = [T.Launch(dev, rk, T._rank_data(u, Du, ranks, parts, k)) for k, rk in enumerate(ranks)]
    new_ex = lambda: [torch.full((n_ex,), float("nan"), dtype=torch.float64, device=dev) for _ in las]    # noqa: E731
    out, ex = [], new_ex()
    for la, e in zip(las, ex):
        la.fwd_call(1, e)
    out += [f"fwd_ex{k}={sha(e.cpu().numpy())}" for k, e in enumerate(ex)]
    T._all_reduce(ex)
    for la, e in zip(las, ex):
        la.fwd_call(2, e)
    gots = [la.fwd_read() for la in las]
    MEAN, INV = [g["save_mean"] for g in gots[0]], [g["save_invstd"] for g in gots[0]]
    ex = new_ex()
    for k, (la, e) in enumerate(zip(las, ex)):
        la.bwd_args(T.saved_from(ranks[k], None, gots[k])[0], MEAN, INV)
        la.bwd_call(1, e)
    out += [f"bwd_ex{k}={sha(e.cpu().numpy())}" for k, e in enumerate(ex)]
    T._all_reduce(ex)
    for k, (la, e) in enumerate(zip(las, ex)):
        la.bwd_call(2, e)
        out.append(f"rank{k}: {fields(gots[k])} | {fields(la.bwd_read())}")
    print(f"dp {name} pad={pad} {R.family(u)}: " + " ".join(out), flush=True)


def digest():
    dev = torch.device("cuda:0")
    for s in R.geometry_specs() + R.group_specs() + R.flag_specs():
        single(dev, s)
    for name in R.DP_SPLITS:
        for pad in (3, 4):
            data_parallel(dev, name, pad)


if __name__ == "__main__":
    digest()
