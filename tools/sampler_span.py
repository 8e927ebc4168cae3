"""Sampler span of bench.py's timed region, from a `rocprofv3 --kernel-trace --output-format csv` trace of a plain run:
the start of the last exact-sampler call's first kernel up to the start of the `shuffle_gather_kernel` behind it (the
timed region opens with that call), and each sampler kernel inside it.
usage: python3 tools/sampler_span.py PATH/run_kernel_trace.csv"""
import csv
import json
import sys

SAMPLER = ("slab_begin_kernel", "mt_", "slab_", "exact_assign_kernel")


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    return name.split("(")[0].split("<")[0]


rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
rows.sort()
shuffles = [i for i, r in enumerate(rows) if r[2].endswith("shuffle_gather_kernel")]
end = shuffles[-1]
i = end - 1
while i >= 0 and not rows[i][2].startswith("slab_begin_kernel"):
    i -= 1
call = [r for r in rows[i:end] if r[2].startswith(SAMPLER)]
per = {}
for s, e, n in call:
    per.setdefault(n, []).append((e - s) / 1e3)
print(json.dumps({"span_us": (rows[end][0] - rows[i][0]) / 1e3,
                  "kernels_us": {n: [round(t, 1) for t in v] for n, v in per.items()},
                  "busy_us": round(sum(e - s for s, e, _ in call) / 1e3, 1)}, indent=1))
