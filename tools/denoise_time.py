#!/usr/bin/env python3
"""Feature-preserving denoising (smg_denoise_*) on one GPU: ms per filter (and per filter iteration), ms per update and per outer iteration, loop
entries of the inner solves, the stationary loop against PCG, and the normal error before and after on a noisy copy of the mesh.

    python tools/denoise_time.py [--legs bunny,bunny2] [--iters 10] [--reps 5]

bunny: bunny_15K_init (15 804 vertices) after normalize_unit_area; bunny2: its 2 x mid-point subdivision (252 834 vertices).  The input is the
mesh plus 0.2 x mean edge x N(0, 1) per coordinate (numpy default_rng(0)); the scalar hierarchy is mg_precompute(V_noisy, F, 0.25, 500, 1).
Defaults of smg_denoise_params (sigma_s by the rule, sigma_r = 0.35, fidelity = 1, 20 filter iterations), default inner options (tolerance
1e-8 |b_0|).  Every timed call does the same work (the object keeps no positions); median of --reps after a warm-up call, host clock around a
call that ends in a synchronise.  Also prints the algorithmic bytes of the kernels (the byte model of DESIGN.md section 24)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, reps):
    ts, out = [], None
    for rep in range(reps + 1):
        t1 = time.perf_counter()
        out = fn()
        if rep:
            ts.append(1e3 * (time.perf_counter() - t1))
    return float(np.median(ts)), out


def face_normals(V, F):
    N = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    return N / np.linalg.norm(N, axis=1, keepdims=True)


def mean_angle_deg(a, b):
    return float(np.degrees(np.mean(np.arccos(np.clip(np.sum(a * b, axis=1), -1.0, 1.0)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="bunny,bunny2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import surface_multigrid_code_amd as smg
    from oracle import mesh_np as M
    for name in args.legs.split(","):
        V, F = M.read_smgm("bunny_15K_init.smgm")
        if name == "bunny2":
            V, F, _ = M.subdivision_hierarchy(V, F, 2)
            V, F = np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32)
        Vc = M.normalize_unit_area(V, F)
        n, nF = V.shape[0], F.shape[0]
        edge = float(np.mean([np.linalg.norm(Vc[F[:, i]] - Vc[F[:, (i + 1) % 3]], axis=1) for i in range(3)]))
        Vn = Vc + 0.2 * edge * np.random.default_rng(0).standard_normal(Vc.shape)
        clean = face_normals(Vc, F)
        t0 = time.perf_counter()
        mg = smg.mg_precompute(Vn, F, 0.25, 500, 1)
        t_h = time.perf_counter() - t0
        t0 = time.perf_counter()
        dn = smg.Denoiser(mg, Vn, F)
        t_c = time.perf_counter() - t0
        iters_f = dn.params.normal_iters
        print("%s: %d vertices, %d faces, %d levels; hierarchy %.2f s, create (neighbourhoods, one precompute) %.2f s, sigma_s %.4e, device memory of the "
              "object %.1f MB" % (name, n, nF, mg.n_levels, t_h, t_c, dn.sigma_s, dn.device_bytes() / 1e6), flush=True)
        med, m = median_ms(lambda: dn.filter(), args.reps)
        dn.set_filter(normal_iters=0)
        med0, _ = median_ms(lambda: dn.filter(), args.reps)
        dn.set_filter(normal_iters=iters_f)
        dn.filter()
        print("  filter %2d iterations  %9.3f ms / call  %8.3f ms / iteration  (0 iterations, the copies alone: %.3f ms)   normal error %.2f -> %.2f degrees"
              % (iters_f, med, (med - med0) / max(iters_f, 1), med0, mean_angle_deg(face_normals(Vn, F), clean), mean_angle_deg(m, clean)), flush=True)
        for pcg in (1, 0):
            dn.set_solver(pcg)
            tag = "PCG" if pcg else "stationary"
            for iters in (args.iters, 0):
                med, (X, E, cyc) = median_ms(lambda: dn.update(max_iter=iters), args.reps)
                if iters:
                    print("  update %-10s %2d iterations  %9.3f ms / call  %8.3f ms / iteration   loop entries %s   E %.4e -> %.4e   normal error %.2f degrees"
                          % (tag, iters, med, med / iters, list(map(int, cyc)), E[0], E[-1], mean_angle_deg(face_normals(X, F), clean)), flush=True)
                else:
                    print("  update %-10s  0 iterations  %9.3f ms / call  (the copies and one local step)" % (tag, med), flush=True)
        # byte model: every array the kernel needs, once (pairs = the entries of N)
        pairs = int(smg._lib.load().smg_mesh_face_neighbours(np.ascontiguousarray(F, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int)), nF, n, None, None))
        filt = 4 * (nF + 1) + 4 * pairs + 56 * nF + 24 * nF                      # the CSR, c, A and m in; m out
        proj = 12 * nF + 24 * nF + 24 * nF + 24 * n + 8 * nF + 72 * nF           # F, w, m, X in; the energy term and the 9 shares out
        rhs = 4 * (n + 1) + 12 * nF + 72 * nF + 8 * n + 48 * n + 24 * n + 16 * n   # corner lists, shares, M, V and X in; B and the two terms out
        print("  neighbourhoods: %d entries, %.2f per face; algorithmic bytes per launch: k_denoise_filter %.1f MB, k_denoise_project %.1f MB, "
              "k_pd_vertices %.1f MB" % (pairs, pairs / nF, filt / 1e6, proj / 1e6, rhs / 1e6), flush=True)
        del dn, mg


if __name__ == "__main__":
    main()
