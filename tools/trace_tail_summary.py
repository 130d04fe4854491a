#!/usr/bin/env python
"""The backward tail of the replayed step out of a rocprofv3 kernel trace (tools/gpu_trace_overlap.sh writes kernel_trace.csv):
    python tools/trace_tail_summary.py <dir with kernel_trace.csv> [label]
Over every replayed step (staging launch to staging launch; the steps that carry the whole-table flush are left out by their
length): the embedding grad-input launch and the batched grad-weight launch (two kernels, or k_g2_xw where the trainer issues
them as one), the time from the start of the first to the end of the last of them, and when each chain reaches the join
(main: end of the grad-weight work; side: end of the last kernel it started before that), as median (min .. max) in
microseconds from the step's start."""
import csv
import statistics
import sys

O = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else O
rows = list(csv.DictReader(open(f"{O}/kernel_trace.csv")))
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?") + "/" + r.get("Stream_Id", "?"))
            for r in rows)
st = [i for i, e in enumerate(ev) if "k_stage_batch_next" in e[2]]
steps = [ev[a:b + 1] for a, b in zip(st, st[1:])]          # (the next step's staging launch closes the step)
length = [(s[-1][0] - s[0][0]) / 1e3 for s in steps]
med_len = statistics.median(length)
got = {k: [] for k in ("grad-input", "grad-weight", "fused", "first start -> last end", "main at the join", "side at the join",
                       "main - side at the join", "k_cgc_mid_bwd", "step length")}
for s, ln in zip(steps, length):
    if ln > 1.3 * med_len:
        continue
    s = s[:-1]
    t0 = s[0][0]
    side_q = next((e[3] for e in s if "k_lazy_flush" in e[2]), None)
    if side_q is None:
        continue
    main = [e for e in s if e[3] != side_q]
    side = [e for e in s if e[3] == side_q]
    xw = [e for e in main if "k_g2_xw" in e[2]]
    tn = [e for e in main if "k_g2_tn_dual" in e[2]]
    nt = [e for e in main if "k_g2_nt<64, 64, 3>" in e[2]]
    if xw:
        first, last = xw[-1], xw[-1]
        got["fused"].append((last[1] - first[0]) / 1e3)
    elif tn and nt:
        first, last = nt[-1], tn[-1]
        got["grad-input"].append((first[1] - first[0]) / 1e3)
        got["grad-weight"].append((last[1] - last[0]) / 1e3)
    else:
        continue
    got["first start -> last end"].append((last[1] - first[0]) / 1e3)
    got["main at the join"].append((last[1] - t0) / 1e3)
    # (the launch behind the join may run on the queue the side chain uses: the side chain is what started before the main chain ended)
    got["side at the join"].append((max(e[1] for e in side if e[0] < last[1]) - t0) / 1e3)
    got["main - side at the join"].append(got["main at the join"][-1] - got["side at the join"][-1])
    got["k_cgc_mid_bwd"] += [(e[1] - e[0]) / 1e3 for e in main if "k_cgc_mid_bwd" in e[2]]
    got["step length"].append(ln)
n = len(got["main at the join"])
print(f"# {label}: {n} replayed steps (of {len(steps)}; median step length by the trace {med_len:.1f} us); median (min .. max), us")
for k, v in got.items():
    if v:
        print(f"{k:26s} {statistics.median(v):7.1f}  ({min(v):.1f} .. {max(v):.1f})")
