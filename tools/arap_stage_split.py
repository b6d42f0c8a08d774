#!/usr/bin/env python3
"""Per-iteration kernel time of smg_arap_solve from a rocprofv3 kernel trace (rocpd sqlite) of tools/arap_time.py:

    rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/arap_time.py --legs C3 --reps 2 --stationary 0
    python tools/arap_stage_split.py DIR/t_results.db

A call runs from k_arap_set_handles to the last k_fixed_sum_final before the next k_arap_set_handles; the launches that are not k_arap_* / k_fixed_sum_*
inside a call are the inner solves.  Prints, for the calls with the most iterations, the median per call of every stage and the same per iteration
(iterations = k_arap_rhs launches)."""
import collections
import re
import sqlite3
import sys

cur = sqlite3.connect(sys.argv[1]).cursor()
q = ("select s.display_name, d.start, d.end from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start")
rows = [(re.sub(r"[<(].*", "", n).replace("void ", "").replace("smg::", ""), s, e) for n, s, e in cur.execute(q)]
STAGE = {"k_arap_rotations": "rotations", "k_arap_rhs": "rhs", "k_fixed_sum_part": "energy", "k_fixed_sum_final": "energy",
         "k_arap_rows": "layout", "k_arap_columns": "layout", "k_arap_set_handles": "layout"}
calls, cur_call = [], None
for nm, s, e in rows:
    if nm == "k_arap_set_handles":
        cur_call = collections.defaultdict(float)
        cur_call["t0"] = s
        calls.append(cur_call)
    if cur_call is None:
        continue
    if nm in STAGE:
        cur_call[STAGE[nm]] += (e - s) / 1e6
        cur_call["t1"] = e
        cur_call["iters"] += nm == "k_arap_rhs"
        cur_call["solve"] += cur_call.pop("pending", 0.0)
    else:
        cur_call["pending"] += (e - s) / 1e6       # counted as inner solve once a later launch of the call's own kernels shows the call went on
most = max(int(c["iters"]) for c in calls)
sel = [c for c in calls if int(c["iters"]) == most]
med = lambda k: sorted(c[k] for c in sel)[len(sel) // 2]   # noqa: E731
print("%d calls of %d iterations" % (len(sel), most))
for k in ("rotations", "rhs", "energy", "layout", "solve"):
    print("  %-10s %8.3f ms / call  %7.4f ms / iteration" % (k, med(k), med(k) / most))
busy = sum(med(k) for k in ("rotations", "rhs", "energy", "layout", "solve"))
span = sorted((c["t1"] - c["t0"]) / 1e6 for c in sel)[len(sel) // 2]
print("  kernel busy %.3f ms, first-to-last span %.3f ms; the new kernels are %.1f %% of the kernel time" % (busy, span, 100 * (busy - med("solve")) / busy))
