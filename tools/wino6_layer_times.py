"""Per-layer time of the Winograd dilated layers from a rocprofv3 kernel trace (--kernel-trace --output-format csv) of the plain bench:
the launches of dilconv_wino6_kernel are taken in start order, six per forward pass (L4 .. L9: dilations 1, 2, 4, 8, 16, 1), and each
layer position gets the median and mean of its launch durations.
usage: python3 tools/wino6_layer_times.py KERNEL_TRACE_CSV [label]"""
import csv
import statistics
import sys

DIL = (1, 2, 4, 8, 16, 1)
rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        if "dilconv_wino6_kernel" in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
rows.sort()
# a pass starts at the launch that follows an EPI 2 launch (<2>: L9 with the head) or at the first one
per = [[] for _ in DIL]
pos = 0
for _, dur, name in rows:
    per[pos].append(dur / 1000.0)
    pos = 0 if "<2>" in name else (pos + 1) % len(DIL)
label = sys.argv[2] if len(sys.argv) > 2 else ""
print(f"# {label} dilconv_wino6_kernel per layer position, us (n launches, median, mean)")
for k, d in enumerate(DIL):
    v = per[k]
    if v:
        print(f"L{k + 4} d={d:2d}  n={len(v):5d}  median {statistics.median(v):7.2f}  mean {statistics.fmean(v):7.2f}")
