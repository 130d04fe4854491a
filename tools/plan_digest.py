"""Digest of what the plan builder (plan.py) produces, to hold two versions of it against each other:

    python tools/plan_digest.py > digest.txt        (on a GPU; `diff` the outputs of the two versions)

Per case it prints the launch names of plan.fwd_steps / plan.bwd_steps and a SHA-256 over every Plan.call of the plan in
creation order: the entry point, the launch name and every argument.  Plain arguments go in by value; an argument block passed
by reference is walked through its _fields_ (nested blocks and arrays included); every pointer — a c_void_p field or a
c_void_p argument — is replaced by the ordinal of that address's first appearance in the case, so that two runs whose
allocator hands out other addresses agree.  The hash also covers which recorded call stands where in the two step lists,
plan.grad_slabs, the number of deferred grad-weight steps and n_wshadow_steps.

Trajectory cases also run three TrainStep.step calls on seeded synth.make_dataset batches and hash the predictions, the BCE
figures, all dense parameters, the Adam moments and the table.  (The regularisation figure is left out: it is summed by atomics
and differs in its last bits between two runs of the same code.)
"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cdcmdr_amd import plan as P  # noqa: E402

DEV = torch.device("cuda:0")
CFG = types.SimpleNamespace(use_atten=False, use_dcn=False)
GOLDEN = ["g2_ple3", "g2_mmoe4", "g2_mmoe8", "g2_dcn13", "g2_dcnv2_mix", "g2_dcnv2_stacked", "g2_star5_all", "g2_star30_all",
          "g11_deepfm", "g12_ple3_atten", "g12_mmoe4_atten_nores", "g12_star3_atten", "g13_autoint", "g13_adasparse", "g16_pepnet",
          "g16_epnet", "g13_epnet_single"]

# ---------------------------------------------------------------------------------------------- recording
_calls = {}           # id(plan) -> [(entry point, launch name, args, the step Plan.call returned)]
_plan_call = P.Plan.call


def _recording_call(self, fn_name, *args, **kw):
    run = _plan_call(self, fn_name, *args, **kw)
    _calls.setdefault(id(self), []).append((fn_name, kw.get("what") or fn_name, args, run))
    return run


P.Plan.call = _recording_call


def _canon(v, ctype, ptr):
    if ctype is C.c_void_p:
        return ptr(v)
    if isinstance(ctype, type) and issubclass(ctype, C.Structure):
        return [_canon(getattr(v, n), t, ptr) for n, t, *_ in ctype._fields_]
    if isinstance(ctype, type) and issubclass(ctype, C.Array):
        return [_canon(v[i], ctype._type_, ptr) for i in range(ctype._length_)]
    return getattr(v, "value", v)


def digest(plan):
    ords = {}

    def ptr(v):
        v = getattr(v, "value", v)
        if not v:
            return "null"
        return "p%d" % ords.setdefault(int(v), len(ords))

    rec = _calls.get(id(plan), [])
    out = []
    for fn_name, what, args, _ in rec:
        types_ = getattr(plan.lib, fn_name).argtypes
        row = [fn_name, what]
        for a, t in zip(args, types_):
            if hasattr(a, "_obj"):                     # byref(block), whether the signature says POINTER(block) or c_void_p
                row.append(_canon(a._obj, type(a._obj), ptr))
            else:
                row.append(_canon(a, t, ptr))
        out.append(row)
    index = {id(run): i for i, (_, _, _, run) in enumerate(rec)}
    out.append(["fwd"] + [index.get(id(s), -1) for s in plan.fwd_steps])
    out.append(["bwd"] + [index.get(id(s), -1) for s in plan.bwd_steps])
    out.append(["slabs"] + [(ptr(k), ptr(v[0]), v[1], v[2]) for k, v in plan.grad_slabs.items()])
    out.append(["tail", len(plan.deferred_dw_steps), plan.n_wshadow_steps])
    return hashlib.sha256(repr(out).encode()).hexdigest()


def names(steps):
    return ",".join("comm" if getattr(s, "is_comm", False) else getattr(s, "what", "host") for s in steps)


def report(case, plan):
    print(f"{case} fwd {names(plan.fwd_steps)}")
    print(f"{case} bwd {names(plan.bwd_steps)}")
    print(f"{case} calls {len(_calls.get(id(plan), []))} sha256 {digest(plan)}")
    _calls.pop(id(plan), None)


def tensor_hash(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- cases
def plan_case(case, make, B, **kw):
    """digest only: the model's own plan (what forward() runs), f32 and bf16, train and eval"""
    for prec in ("f32", "bf16"):
        for train in (True, False):
            torch.manual_seed(1)
            m = make().to(DEV).set_precision(prec)
            m.train(train)
            report(f"{case}/{prec}/{'train' if train else 'eval'}", m.plan_holder(B, **kw).plan)


def dp_case(case, make, B, dp):
    """digest only: the training step's plan under data parallelism with one forced rank (global-batch BatchNorm statistics)"""
    from cdcmdr_amd.optim import FusedAdam
    for prec in ("f32", "bf16"):
        for train in (True, False):
            torch.manual_seed(1)
            m = make().to(DEV).set_precision(prec)
            m.train(train)
            opt = FusedAdam(m, table_mode="lazy")
            plan = P.Plan(DEV, B, precision=prec, training=train, dropout=0.0, seed=0, step_dev=opt.step_dev, grad_arena=opt.grad_arena,
                          dist=dp, defer_dw_reduce=False)
            emb = m.embedding.describe(plan)
            outs, _, _ = m.describe(plan, emb)
            plan.finalize(outs)
            report(f"{case}/{prec}/{'train' if train else 'eval'}", plan)


def train_case(case, make, fd, B, prec, mode, n_domain, domain_idx, seed):
    """digest of the training step's plan, then three steps on seeded batches"""
    from cdcmdr_amd.optim import FusedAdam
    from cdcmdr_amd.synth import make_dataset
    from cdcmdr_amd.trainer import TrainStep
    torch.manual_seed(seed)
    m = make().to(DEV).set_precision(prec)
    m.seed = seed
    opt = FusedAdam(m, table_mode="lazy")
    t0 = time.perf_counter()
    ts = TrainStep(m, opt, B, mode=mode)
    sys.stderr.write(f"{case}: TrainStep built in {time.perf_counter() - t0:.3f} s (host)\n")
    report(case, ts.plan)
    X, y = make_dataset(3 * B, fd, n_domain=n_domain, domain_idx=domain_idx, seed=2000 + seed)
    for s in range(3):
        sl = slice(s * B, (s + 1) * B)
        Xs = torch.from_numpy(X[sl]).to(DEV)
        bce, _ = ts.step(Xs, torch.from_numpy(y[sl]).to(DEV), torch.from_numpy(X[sl, domain_idx].astype(np.int64)).to(DEV))
        torch.cuda.synchronize()
        print(f"{case} step {s} bce {float(bce.item())!r} pred {tensor_hash([ts.out.tensor()])}")
    ts.check_ids()
    osd = opt.state_dict()["state"]                   # (flushes the lazy table)
    sd = m.state_dict()
    table = "embedding.embedding_dict.weight"
    print(f"{case} dense {tensor_hash([sd[k] for k in sorted(sd) if k != table])}")
    print(f"{case} moments {tensor_hash([osd[k][w] for k in sorted(osd) for w in ('exp_avg', 'exp_avg_sq')])}")
    print(f"{case} table {tensor_hash([sd[table]])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    only = ap.parse_args().only
    from test_gpu_models_golden import FD, FD13, build
    from cdcmdr_amd.dist import DataParallel
    from cdcmdr_amd.model.dcnv2 import DCNv2
    from cdcmdr_amd.model.mmoe import MMoE
    from cdcmdr_amd.model.ple import PLE
    from cdcmdr_amd.model.star import STAR
    fd25 = list(FD)
    fd25[2] = 25
    fd_star30 = [50, 3000, 11, 700, 30, 29]
    fd_dist = [30, 2000, 7, 300, 3]
    fd_big = [1000] * 26
    star30 = lambda: STAR(fd_star30, 16, 30, (64, 32, 16), domain_idx=4, dropout=0.0)      # noqa: E731
    big = lambda: PLE(fd_big, 16, 3, 2, 2, ((256, 128), (64,)), (64, 32), 0.2, CFG)        # noqa: E731
    cases = []
    for name in GOLDEN:
        kw = {"tag": "all"} if "star" in name else {}
        cases.append((name, lambda name=name, kw=kw: plan_case(name, lambda: build(name), 96, **kw)))
    cases += [
        ("star5_grouped", lambda: plan_case("star5_grouped", lambda: STAR(FD, 4, 5, (32, 16, 8), dropout=0.0), 96, tag="grouped", grouped=True)),
        ("ple25", lambda: plan_case("ple25", lambda: PLE(fd25, 4, 25, 2, 2, ((32, 16), (8,)), (8, 4), dropout=0.0, config=CFG), 384)),
        ("star30", lambda: plan_case("star30", star30, 1024, tag="all")),
        ("star30_grouped", lambda: plan_case("star30_grouped", star30, 1024, tag="grouped", grouped=True)),
    ]
    dp = []

    def the_dp():
        if not dp:
            os.environ.setdefault("MASTER_PORT", "29731")
            dp.append(DataParallel(backend="gloo", force=True))
        return dp[0]
    cases += [
        ("dp_mmoe", lambda: dp_case("dp_mmoe", lambda: MMoE(fd_dist, 8, 3, 4, (32, 16), (8,), dropout=0.0), 96, the_dp())),
        ("dp_mmoe_wide", lambda: dp_case("dp_mmoe_wide", lambda: MMoE(fd_big, 16, 3, 4, (256, 128, 64), (64, 32), dropout=0.0, config=CFG),
                                         4096, the_dp())),
        ("dp_ple64", lambda: dp_case("dp_ple64", lambda: PLE(fd_dist, 8, 3, 1, 1, ((32,), (64,)), (64, 32), dropout=0.0), 96, the_dp())),
        ("train_ple_4096", lambda: train_case("train_ple_4096", big, fd_big, 4096, "bf16", "multi", 3, 10, 11)),
        ("train_ple_8320", lambda: train_case("train_ple_8320", big, fd_big, 8320, "bf16", "multi", 3, 10, 12)),
        ("train_mmoe8", lambda: train_case("train_mmoe8", lambda: build("g2_mmoe8"), FD, 96, "f32", "multi", 3, 2, 13)),
        ("train_dcnv2_mix", lambda: train_case("train_dcnv2_mix", lambda: DCNv2(FD13, 4, 3, (32, 16, 8), dropout=0.0, low_rank=8, num_experts=4),
                                               FD13, 96, "bf16", "single", 3, 4, 14)),
        ("train_star30_grouped", lambda: train_case("train_star30_grouped", star30, fd_star30, 1024, "bf16", "star", 30, 4, 15)),
    ]
    failed = 0
    for name, run in cases:
        if only in name:
            try:
                run()
            except Exception as e:  # noqa: BLE001
                failed += 1
                print(f"{name} ERROR {type(e).__name__}: {e}")
            sys.stdout.flush()
    if dp:
        dp[0].close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
