"""Per-step launch boundaries of the Goku Adam step from a rocprofv3 --kernel-trace CSV:
    python tools/step_gaps.py RUN_kernel_trace.csv [LAST_N_DISPATCHES]
Takes the last N dispatches of the step kernels (k_chol_flow, k_grad, k_reduce_items; default
600: the replayed, timed part of a bench run), and prints each kernel's count and mean duration
and the mean idle gap of every boundary kind (end of one kernel to the start of the next)."""
import csv
import sys
from collections import defaultdict

NAMES = ("k_chol_flow", "k_grad", "k_reduce_items")


def short(name):
    for k in NAMES:
        if k in name:
            return k
    return None


def main():
    path = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 600
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if k:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k))
    rows.sort()
    rows = rows[-last:]
    dur, gap = defaultdict(list), defaultdict(list)
    for i, (s, e, k) in enumerate(rows):
        dur[k].append(e - s)
        if i:
            ps, pe, pk = rows[i - 1]
            gap[f"{pk} -> {k}"].append(s - pe)
    span = rows[-1][1] - rows[0][0]
    nflow = len(dur["k_chol_flow"])
    print(f"{len(rows)} dispatches, {nflow} flows, {span / 1e3 / max(nflow, 1):.2f} us per flow (first start to last end)")
    for k in NAMES:
        if dur[k]:
            v = sorted(dur[k])
            print(f"  {k:16s} n {len(v):5d}  mean {sum(v) / len(v) / 1e3:8.2f} us  median {v[len(v) // 2] / 1e3:8.2f} us")
    for k, v in sorted(gap.items()):
        v = sorted(v)
        print(f"  gap {k:34s} n {len(v):5d}  mean {sum(v) / len(v) / 1e3:7.2f} us  median {v[len(v) // 2] / 1e3:7.2f} us")


if __name__ == "__main__":
    main()
