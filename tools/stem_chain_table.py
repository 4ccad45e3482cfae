"""Per-step kernel time of the ResNet stem chain from a rocprofv3 kernel trace (csv) of
the eager step (`rocprofv3 --kernel-trace --stats ... -- python bench.py --graph 0`):

    python tools/stem_chain_table.py TRACE_kernel_trace.csv [STEPS]

The chain's launches are found by position, per stream: what follows a stem_x6_fwd_kernel
up to the pool forward, and what leads from the pool backward to the stem weight
gradient's final sum.  Prints, per encoder (3 input channels: depth, 6: pose), the mean
duration in microseconds of every launch of the chain over the last STEPS steps (default
20) and the chain totals."""
import csv
import re
import sys
from collections import defaultdict

FWD_END = ("maxpool_fwd", "bn_relu_pool")
SHORT = re.compile(r"(?:void )?(?:\(anonymous namespace\)::)?([A-Za-z0-9_]+)(<[^>]*>)?")


def short(name: str) -> str:
    m = SHORT.match(name)
    return (m.group(1) + (m.group(2) or "")) if m else name


def main():
    path = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    streams = defaultdict(list)
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            streams[(r.get("Stream_Id"), r["Queue_Id"])].append(
                (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    chains = defaultdict(list)   # (encoder, "fwd" | "bwd") -> [[(name, ns), ...] per step]
    for seq in streams.values():
        seq.sort()
        names = [k[2] for k in seq]
        for i, n in enumerate(names):
            if n.startswith("stem_x6_fwd_kernel"):
                enc = "pose" if "<6" in n else "depth"
                j = i
                while j + 1 < len(seq) and not names[j].startswith(FWD_END) and j - i < 6:
                    j += 1
                chains[(enc, "fwd")].append([(names[k], seq[k][1] - seq[k][0]) for k in range(i, j + 1)])
            elif n.startswith("stem_x6_wgrad_tr_kernel"):
                enc = "pose" if "<6" in n else "depth"
                j = i
                while j > 0 and not names[j].startswith("maxpool_bwd") and i - j < 6:
                    j -= 1
                chains[(enc, "bwd")].append([(names[k], seq[k][1] - seq[k][0]) for k in range(j, i + 2)])
    total = 0.0
    for key in sorted(chains):
        runs = chains[key][-steps:]
        shape = [n for n, _ in runs[-1]]
        runs = [r for r in runs if [n for n, _ in r] == shape]
        print(f"{key[0]} stem, {key[1]} ({len(runs)} steps)")
        sub = 0.0
        for c, n in enumerate(shape):
            us = sum(r[c][1] for r in runs) / len(runs) / 1e3
            sub += us
            print(f"  {n:58s} {us:8.1f} us")
        print(f"  {'chain':58s} {sub:8.1f} us")
        total += sub
    print(f"stem chains, both encoders, per step: {total:.1f} us")


if __name__ == "__main__":
    main()
