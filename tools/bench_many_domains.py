"""ms/step of the fast path with one tower per domain (the reference's "split" grouping, config.py:63-72): PLE-25, PLE-50 and
MMoE-50 at B = 4096, STAR-50 grouped at B = 16384, 26 fields x vocab 1M, emb_dim 16, the reference's dims.  Single GPU.
  python tools/bench_many_domains.py [ple25 ple50 mmoe50 star50]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_configs import run  # noqa: E402


def main():
    which = sys.argv[1:] or ["ple25", "ple50", "mmoe50", "star50"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dom = 10
    for name in which:
        n = int(name[-2:])
        fd = [1_000_000] * 26
        fd[dom] = n
        with torch.device(dev):
            if name.startswith("ple"):
                from cdcmdr_amd.model.ple import PLE
                m, mode, B = PLE(fd, 16, n, 2, 2, ((256, 128), (64,)), (64, 32), dropout=0.2), "multi", 4096
            elif name.startswith("mmoe"):
                from cdcmdr_amd.model.mmoe import MMoE
                m, mode, B = MMoE(fd, 16, n, 4, (256, 128, 64), (64, 32), dropout=0.2), "multi", 4096
            else:
                from cdcmdr_amd.model.star import STAR
                m, mode, B = STAR(fd, 16, n, (256, 128, 64, 32), domain_idx=dom, dropout=0.2), "star", 16384
        run(f"{name}: 26x1M D16 B{B}", m, mode, B, fd, n, dom)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
