#!/usr/bin/env python3
"""Per-step kernel time of smg_membrane_step from a rocprofv3 kernel trace (rocpd sqlite) of tools/membrane_time.py:

    rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/membrane_time.py --legs bunny --reps 2 --host-iters 0
    python tools/membrane_stage_split.py DIR/t_results.db

A step runs from k_membrane_pressure_faces to the launch before the next one.  Inside it a Newton iteration starts at k_membrane_faces<2>;
k_membrane_faces<2>, k_membrane_matrix and k_membrane_gradient are the assembly; the kernels of the value-only re-precompute and of the solve are
not told apart by name alone, so every launch that is not k_membrane_* / k_fixed_sum_* counts as "re-precompute + solve"; k_membrane_trial, the energy-only k_membrane_faces<0>, k_membrane_dot3 and the
reductions are the line search.  Prints the median per step of every stage over the steps with the most Newton iterations."""
import collections
import re
import sqlite3
import sys

cur = sqlite3.connect(sys.argv[1]).cursor()
q = ("select s.display_name, d.start, d.end from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start")
rows = []
for n, s, e in cur.execute(q):
    mode = re.search(r"k_membrane_faces<(\d)", n)
    nm = re.sub(r"[<(].*", "", n).replace("void ", "").replace("smg::", "")
    rows.append((nm + (mode.group(1) if mode else ""), s, e))
STAGE = {"k_membrane_faces2": "assembly", "k_membrane_matrix": "assembly", "k_membrane_gradient": "assembly", "k_membrane_pressure_faces": "pressure",
         "k_membrane_pressure": "pressure", "k_membrane_trial": "line search", "k_membrane_faces0": "line search", "k_membrane_dot3": "line search",
         "k_fixed_sum_part": "line search", "k_fixed_sum_final": "line search"}
steps, cur_step = [], None
for nm, s, e in rows:
    if nm == "k_membrane_pressure_faces":
        cur_step = collections.defaultdict(float)
        cur_step["t0"] = s
        steps.append(cur_step)
    if cur_step is None:
        continue
    if nm in STAGE:
        cur_step[STAGE[nm]] += (e - s) / 1e6
        cur_step["t1"] = e
        cur_step["iters"] += nm == "k_membrane_faces2"
        cur_step["fix kernel"] += (e - s) / 1e6 if nm == "k_membrane_faces2" else 0.0
        cur_step["re-precompute + solve"] += cur_step.pop("pending", 0.0)
    else:
        cur_step["pending"] += (e - s) / 1e6      # counted once a later membrane launch shows the step went on
most = max(int(c["iters"]) for c in steps)
sel = [c for c in steps if int(c["iters"]) == most]
med = lambda k: sorted(c[k] for c in sel)[len(sel) // 2]   # noqa: E731
print("%d steps of %d Newton iterations" % (len(sel), most))
keys = ("pressure", "assembly", "re-precompute + solve", "line search")
for k in keys + ("fix kernel",):
    print("  %-22s %8.3f ms / step  %7.4f ms / Newton iteration%s" % (k, med(k), med(k) / most, "   (part of assembly)" if k == "fix kernel" else ""))
busy = sum(med(k) for k in keys)
span = sorted((c["t1"] - c["t0"]) / 1e6 for c in sel)[len(sel) // 2]
print("  kernel busy %.3f ms, first-to-last span %.3f ms" % (busy, span))
