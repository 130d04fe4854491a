"""Times the training step with loss weights beside the unweighted step of the same tree.

bench.py's flagship shape and loop: PLE-3, 26 fields x vocab 1 M, emb_dim 16, batch 4096, bf16, lazy table, the step replayed as one
hipGraph with the next batch named one step ahead.  Two steps on models of their own, identical seeds:
    plain     TrainStep(...)                                                        the step bench.py times
    weighted  TrainStep(..., loss_weights=LossWeights(row=True, domain_weight=..., domain_idx=10, pos_weight=2.5)), weight= every step
Both are brought to the lazy table's steady state like bench.py does, then timed alternately (plain, weighted, plain, ...): `--rounds`
brackets of `--steps` steps each, a host clock between two device synchronisations.  After that a few eager steps through
TrainStep.profile() count the launches of a step, the staging launches included.  Needs a GPU: there is no fallback.  Prints one
JSON line; `--trace-only N` runs N weighted steps and nothing else (for a kernel trace of cdc_stage_weights).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from cdcmdr_amd.optim import FusedAdam  # noqa: E402
from cdcmdr_amd.synth import make_dataset  # noqa: E402
from cdcmdr_amd.trainer import LossWeights, TrainStep  # noqa: E402

DOMAIN_IDX, POOL = 10, 256


def build(args, weighted, dev):
    model, field_dims = bench.build_model(args, dev)
    opt = FusedAdam(model, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-8, table_mode="lazy", flush_every=args.flush_every)
    lw = None
    if weighted:
        dom_w = np.ones(field_dims[DOMAIN_IDX], dtype=np.float32)
        dom_w[:3] = (0.5, 2.0, 1.25)                                # the synthetic stream has three domains
        lw = LossWeights(row=True, domain_weight=dom_w, domain_idx=DOMAIN_IDX, pos_weight=2.5)
    return TrainStep(model, opt, args.batch, mode="multi", use_graph=True, loss_weights=lw), opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", type=int, default=0)
    a = ap.parse_args()
    args = argparse.Namespace(vocab=1_000_000, fields=26, embed_dim=16, dropout=0.2, precision="bf16", atten=0, batch=4096, flush_every=64)
    if not torch.cuda.is_available():
        raise SystemExit("weighted_step_bench needs a GPU")
    dev = torch.device("cuda", 0)
    B = args.batch
    Xr, yr = make_dataset(B * POOL, [args.vocab] * args.fields, n_domain=3, domain_idx=DOMAIN_IDX, seed=2000, dist="uniform")
    Xd = torch.from_numpy(Xr).to(dev).view(POOL, B, -1)
    yd = torch.from_numpy(yr).to(dev).view(POOL, B)
    gd = torch.from_numpy(Xr[:, DOMAIN_IDX].astype(np.int64)).to(dev).view(POOL, B)
    wd = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 3.0, size=(POOL, B)).astype(np.float32)).to(dev)

    def run(ts, n, cursor):
        for _ in range(n):
            j = cursor[0] % POOL
            cursor[0] += 1
            kw = {"weight": wd[j]} if ts.loss_weights is not None else {}
            ts.step(Xd[j], yd[j], gd[j], next_X=Xd[cursor[0] % POOL], **kw)

    def timed(ts, n, cursor):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(ts, n, cursor)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    kinds = ("weighted",) if a.trace_only else ("plain", "weighted")
    steps, cursors = {}, {}
    for kind in kinds:
        steps[kind], cursors[kind] = build(args, kind == "weighted", dev), [0]
        ts, opt = steps[kind]
        run(ts, a.trace_only or (args.flush_every + int(opt.scalars.shape[0]) + 64 + 20), cursors[kind])     # bench.py's preroll + warm-up
    torch.cuda.synchronize()
    if a.trace_only:
        return
    ms = {kind: [] for kind in kinds}
    for _ in range(a.rounds):
        for kind in kinds:
            ms[kind].append(round(timed(steps[kind][0], a.steps, cursors[kind]), 4))
    last_bce = {k: float(steps[k][0].loss.item()) for k in kinds}               # of the last timed step
    launches = {}
    for kind in kinds:
        ts = steps[kind][0]
        batches = [(Xd[j], yd[j], gd[j]) for j in range(8)]
        if kind == "weighted":
            orig = ts.step
            ts.step = lambda X, y, g, _o=orig: _o(X, y, g, weight=wd[0])        # profile() hands step() the three batch tensors
        prof = ts.profile(batches, n_steps=10, skip=2)
        launches[kind] = {"per_step": round(sum(v["launches_per_step"] for v in prof.values()), 2),
                          "stage_weights_ms": prof.get("cdc_stage_weights", {}).get("ms_per_step"),
                          "names": {k: round(v["launches_per_step"], 2) for k, v in prof.items() if "bce" in k or "stage" in k or "tower" in k}}
    print(json.dumps({"steps_per_bracket": a.steps, "ms_per_step": ms, "median_ms": {k: float(np.median(v)) for k, v in ms.items()},
                      "launches": launches, "last_bce": last_bce}), flush=True)


if __name__ == "__main__":
    main()
