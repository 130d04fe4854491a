"""Times one CDCTrainer.update_matrix() with the per-domain probe evaluation and with `batched_probe=True`.

CDC on a PLE base at the reference's widths, 26 fields x vocab 100 k, emb_dim 16, bf16, lazy table; 8 and 30 domains at batch sizes
512 and 4096; `n_causal_mask` cut from 50 to 8 so a run stays under a minute (an update then runs 8 + 1 + n + (n + 1) probes).
Both modes start from identical seeds, so they draw the same batches and train the same probe steps; `batched_probe=False` is the
per-domain loop exactly as it was before the batched path existed.  Per mode: one update_matrix() as warm-up (it builds every
plan and step the update needs), then one timed with a host clock between two device synchronisations — regrouping on the host
(`update_group`) included, as a training run pays it.  Needs a GPU: there is no fallback.  Prints one JSON line per point.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdcmdr_amd.cdc_trainer import CDCTrainer  # noqa: E402
from cdcmdr_amd.data import make_domain_loaders  # noqa: E402
from cdcmdr_amd.model.cdc import CDC  # noqa: E402
from cdcmdr_amd.optim import FusedAdam  # noqa: E402

FIELDS, VOCAB, EMB, N_CLUSTER, DOMAIN_IDX = 26, 100_000, 16, 3, 0


def one_update(n_domain, bs, batched, a, dev):
    """-> (seconds of the timed update_matrix(), its matrix_A on the host)"""
    fd = [VOCAB] * FIELDS
    fd[DOMAIN_IDX] = n_domain
    rng = np.random.default_rng(0)
    n = n_domain * bs * a.batches_per_domain
    X = np.stack([rng.integers(0, d, size=n) for d in fd], axis=1).astype(np.int32)
    X[:, DOMAIN_IDX] = np.arange(n) % n_domain                     # every domain holds batches_per_domain full batches
    y = (rng.random((n, 1)) < 0.25).astype(np.int16)
    np.random.seed(1)
    torch.manual_seed(1)
    loaders, seq, w = make_domain_loaders(torch.from_numpy(X), torch.from_numpy(y), bs, dev, DOMAIN_IDX, n_domain)
    cfg = types.SimpleNamespace(ple_n_expert_specific=2, ple_n_expert_shared=2, dataset_name="probe_bench", p_weight=0.5,
                                p_weight_method="linear_decay", p_weight_exp_decay=0.9, old_matrix_weight=0.3, affinity_func="minus",
                                use_atten=False)
    cdc = CDC(fd, EMB, N_CLUSTER, n_domain, "ple", ((256, 128), (64,)), (64, 32), DOMAIN_IDX, domain_cnt_weight=w,
              n_causal_mask=a.n_causal_mask, use_metric=a.metric, device=dev, dropout=0.2, config=cfg).to(dev).set_precision("bf16")
    opt = FusedAdam(cdc.base_model_instance, table_mode="lazy")
    tr = CDCTrainer(cdc, opt, bs, loaders, n_domain, w, seq, batched_probe=batched)
    for _ in range(3):                                              # a few ordinary steps: the moments are not all zero
        Xb, yb = tr.get_domain_data(0)
        tr._step(Xb, yb, "split", domain_i=0)
    tr.update_matrix()                                              # warm-up: plans, steps, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.update_matrix()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, cdc.matrix_A.cpu().clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--domains", type=int, nargs="+", default=[8, 30])
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--n-causal-mask", type=int, default=8)
    ap.add_argument("--batches-per-domain", type=int, default=4)
    ap.add_argument("--metric", choices=["loss", "auc"], default="loss")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bench needs a GPU")
    dev = torch.device("cuda:0")
    os.chdir(tempfile.mkdtemp())                                    # the regrouping dumps its matrices under ./result
    for n_domain in a.domains:
        for bs in a.batch_sizes:
            t_off, A_off = one_update(n_domain, bs, False, a, dev)
            t_on, A_on = one_update(n_domain, bs, True, a, dev)
            probes = a.n_causal_mask + 1 + n_domain + n_domain + 1
            print(json.dumps({"n_domain": n_domain, "bs": bs, "metric": a.metric, "n_causal_mask": a.n_causal_mask, "probes": probes,
                              "per_domain_s": round(t_off, 4), "batched_s": round(t_on, 4), "ratio_per_domain_over_batched": round(t_off / t_on, 3),
                              "matrix_A_max_abs_diff": float((A_on - A_off).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
