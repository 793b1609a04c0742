"""Pass time and launch gaps of a fused fp32 batch step, from a rocprofv3 --kernel-trace CSV of bench.py:
python scripts/scan_step_trace_gaps.py <kernel_trace.csv> [steps]

A step is the run of scan launches (scan_topk_f32_pair_kernel / scan_topk_f32_step_kernel) between two merge_topk launches.
Printed for the last `steps` steps (default 20, the timed ones): launches per step, mean launch duration, mean gap between
consecutive scan launches of a step (start of one minus end of the one before), and the step's span from the first scan's start
to the last scan's end."""
import csv
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
steps_wanted = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps, cur = [], []
for r in rows:
    name = r["Kernel_Name"]
    if "scan_topk_f32_pair_kernel" in name or "scan_topk_f32_step_kernel" in name:
        cur.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name.split("(")[0]))
    elif "merge_topk" in name and cur:
        steps.append(cur)
        cur = []
steps = steps[-steps_wanted:]
durs = [(e - s) / 1e3 for st in steps for s, e, _ in st]
gaps = [(st[i + 1][0] - st[i][1]) / 1e3 for st in steps for i in range(len(st) - 1)]
spans = [(st[-1][1] - st[0][0]) / 1e3 for st in steps]
names = sorted({n for st in steps for _, _, n in st})
print("steps %d, scan launches per step %s, kernels %s" % (len(steps), sorted({len(st) for st in steps}), names))
print("mean scan launch %.2f us (min %.2f, max %.2f)" % (sum(durs) / len(durs), min(durs), max(durs)))
if gaps:
    print("mean gap between consecutive scan launches of a step %.2f us (min %.2f, max %.2f), %d gaps per step"
          % (sum(gaps) / len(gaps), min(gaps), max(gaps), len(gaps) // len(steps)))
print("mean span first scan start .. last scan end %.1f us per step" % (sum(spans) / len(spans)))
