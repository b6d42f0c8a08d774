#!/usr/bin/env python3
"""Per-stage kernel time of heat-method geodesic queries from a rocprofv3 kernel trace (rocpd sqlite) of tools/geodesics_time.py:

    rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/geodesics_time.py --legs C3 --ks 1,8,64 --reps 2 --stationary 0
    python tools/geodesics_stage_split.py DIR/t_results.db [n]

A query runs from k_geo_clear to k_geo_shift; the launches between the scatter and the divergence kernel are the heat solve, those between
the divergence kernel and k_geo_source_mean the Poisson solve.  k is read off the divergence kernel's grid (n = the mesh's vertices, default C3).
Prints the median over the queries of each k."""
import sqlite3, re, sys, collections
db = sqlite3.connect(sys.argv[1]); cur = db.cursor()
q = ("select s.display_name, d.grid_size_x, d.start, d.end from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start")
rows = [(re.sub(r"\(.*", "", n).replace("void ", "").replace("smg::", ""), g, s, e) for n, g, s, e in cur.execute(q)]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1011330
res = collections.defaultdict(lambda: collections.defaultdict(list))
i = 0
while i < len(rows):
    if rows[i][0].startswith("k_geo_clear"):
        j = i; stage = "scatter"; acc = collections.defaultdict(float); k = None; t0 = rows[i][2]
        while j < len(rows):
            nm, g, s, e = rows[j]
            if nm.startswith("k_geo_divergence"):
                k = g // (((n + 255) // 256) * 256); stage = "divergence"
            elif stage == "divergence" and not nm.startswith("k_geo"):
                stage = "poisson"
            elif nm.startswith("k_geo_source_mean"):
                stage = "shift"
            elif stage == "scatter" and not nm.startswith("k_geo"):
                stage = "heat"
            acc[stage] += (e - s) / 1e6
            if nm.startswith("k_geo_shift"):
                acc["span"] = (e - t0) / 1e6
                break
            j += 1
        for kk, v in acc.items(): res[k][kk].append(v)
        i = j + 1
    else:
        i += 1
for k in sorted(res):
    d = res[k]; m = lambda x: sorted(x)[len(x)//2]
    busy = sum(m(d[s]) for s in ("scatter","heat","divergence","poisson","shift"))
    print("k=%2d queries=%d  heat %.2f ms | poisson %.2f ms | scatter %.3f ms | divergence %.3f ms | shift %.3f ms | kernel busy %.2f ms, first-to-last span %.2f ms"
          % (k, len(d["span"]), m(d["heat"]), m(d["poisson"]), m(d["scatter"]), m(d["divergence"]), m(d["shift"]), busy, m(d["span"])))
