"""Step-to-step gap of a bench.py run from a rocprofv3 --kernel-trace CSV.

python tools/step_gap.py <kernel_trace.csv> --steps K [--ms-per-step X] [--out FILE]

A step of the batched path starts with the relax launch, k_batch_rows<.., 1>.
For each of the last K relax launches (the timed steps) the gap runs from the
end of the last engine kernel before it -- the previous step's last kernel;
the runtime's fill and copy kernels and the plan kernels belong to the step
they prepare -- to the relax launch's start: the time in which the batch
kernels do not run.  Printed: the mean / min / max gap, the kernel time that
falls inside the gap (fills, copies, plan kernels), the step's kernel sum and,
if given, ms_per_step of an untraced run beside them.
"""
import argparse
import csv
import json
import re
import statistics

ap = argparse.ArgumentParser()
ap.add_argument("csv")
ap.add_argument("--steps", type=int, required=True)
ap.add_argument("--ms-per-step", type=float, default=None, help="of an untraced run on the same box")
ap.add_argument("--traced-ms-per-step", type=float, default=None, help="of the traced run itself")
ap.add_argument("--out", default=None)
a = ap.parse_args()

RELAX = re.compile(r"k_batch_rows<[^>]*,\s*1>")
# kernels that prepare a step: the runtime's fills / copies, the plan kernels and the sort they call
HEAD = re.compile(r"__amd_rocclr_|k_plan_|rocprim::")

ks = []
for r in csv.DictReader(open(a.csv)):
    ks.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
ks.sort()
relax = [i for i, k in enumerate(ks) if RELAX.search(k[2])]
if len(relax) < a.steps + 1:
    raise SystemExit(f"{len(relax)} relax launches in the trace, need {a.steps + 1}")
timed = relax[-a.steps:]
gaps, inside, sums, plan = [], [], [], []
for n, i in enumerate(timed):
    j = i - 1
    while j >= 0 and HEAD.search(ks[j][2]):
        j -= 1
    gaps.append((ks[i][0] - ks[j][1]) / 1e6)
    inside.append(sum(e - s for s, e, _ in ks[j + 1:i]) / 1e6)
    plan.append(sum(e - s for s, e, nm in ks[j + 1:i] if "k_plan_" in nm or "rocprim::" in nm) / 1e6)
    end = timed[n + 1] if n + 1 < len(timed) else len(ks)
    sums.append(sum(e - s for s, e, nm in ks[i:end] if not HEAD.search(nm)) / 1e6)
out = {
    "steps": a.steps,
    "gap_ms": {"mean": statistics.mean(gaps), "min": min(gaps), "max": max(gaps)},
    "kernel_ms_inside_gap": statistics.mean(inside),
    "plan_kernel_ms_inside_gap": statistics.mean(plan),
    "step_kernel_sum_ms": statistics.mean(sums),
    "ms_per_step_untraced": a.ms_per_step,
    "ms_per_step_traced": a.traced_ms_per_step,
}
text = json.dumps(out, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
