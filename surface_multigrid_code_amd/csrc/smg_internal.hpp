// smg_internal.hpp -- what the translation units behind the C ABI (include/smg.h) share with each other:
//   smg_capi.cpp        errors, the handle (container, setters, introspection), profc mirror, mesh numerics shims
//   smg_precompute.cpp  min_quad_with_fixed_mg_precompute: host sparse algebra, device images, value-only re-precompute, assembly
//   smg_cycle.cpp       mg_VCycle: level vectors, smoothers, launch sequence of a cycle and of the outer residual, pieces, raw interface -- each written
//                       once for T = double / float (vecs<T>(level), the views' vals<T>(), launchers overloaded on the vectors' type)
//   smg_solve.cpp       min_quad_with_fixed_mg_solve: the steps of the solve loops and their graph cache, outer loops (stationary, split-phase, sharded, PCG)
//   smg_sweep_plans.cpp the plan-based Gauss-Seidel sweeps: which one a level uses, building, value refresh, introspection, self-checks
//   smg_hierarchy_io.cpp mg_precompute / mg_precompute_block builders, point queries, .smgh files
// The objects built on a mesh and a caller's hierarchy (smg_geodesics.cpp, smg_arap.cpp, smg_membrane.cpp, smg_param.cpp) share smg_mesh_object.hpp, not this file.
// Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/smg.h"
#include "smg_hier.hpp"
#include "smg_mesh.hpp"

namespace smg {

// ---- errors: the message of the calling thread's last failure (smg_last_error) -----------------------------------------------
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e__ = (expr);                                                                              \
        if (e__ != hipSuccess) return ::smg::fail(SMG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// Nothing may throw across the C ABI: the entry points that allocate host memory run their bodies through this guard.
template <typename Fn>
static int guarded(const char* who, Fn&& body)
{
    try { return body(); }
    catch (const std::bad_alloc&) { return fail(SMG_ERR_ALLOC, "%s: out of host memory", who); }
    catch (const std::exception& e) { return fail(SMG_ERR_INVALID, "%s: %s", who, e.what()); }
    catch (...) { return fail(SMG_ERR_INVALID, "%s: unknown exception", who); }
}

// a handle under construction: destroyed unless release()d (an entry point that builds a hierarchy must not leak it when a later
// step fails or throws)
struct HierarchyOwner {
    smg_hierarchy* h = nullptr;
    explicit HierarchyOwner(smg_hierarchy* p) : h(p) {}
    HierarchyOwner(const HierarchyOwner&) = delete;
    HierarchyOwner& operator=(const HierarchyOwner&) = delete;
    ~HierarchyOwner() { if (h) smg_hierarchy_destroy(h); }
    smg_hierarchy* release() { smg_hierarchy* p = h; h = nullptr; return p; }
};

// ---- device plumbing -----------------------------------------------------------------------------------------------------------
// The current HIP device is a per-thread setting: every entry point that touches the device -- and every worker thread of the
// precompute -- runs on the handle's device, whatever the calling thread had selected (one process may drive several GPUs, and a
// std::thread starts on device 0).  Restores the caller's selection on scope exit.
struct DeviceScope {
    int prev = -1, dev = -1;
    explicit DeviceScope(int d) : dev(d)
    {
        if (d < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) (void)hipSetDevice(d);
    }
    ~DeviceScope() { if (dev >= 0 && prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

inline int env_int(const char* name, int dflt)
{
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

// SMG_TIMING=1: wall-clock of the precompute stages on stderr
struct StageTimer {
    bool on;
    std::chrono::steady_clock::time_point t0;
    StageTimer() : on(env_int("SMG_TIMING", 0) != 0), t0(std::chrono::steady_clock::now()) {}
    void lap(const char* what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[smg timing] %-38s %8.1f ms\n", what, 1e3 * std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    }
};

int ensure_device(smg_hierarchy* h);            // first use of the device by a handle: stream, control block
void drop_graphs(smg_hierarchy* h);             // the cached hipGraphs no longer describe the handle
int check_ready(const smg_hierarchy* h, const char* who);
int check_cycle_opts(const smg_solve_opts& o);  // the option checks of smg_solve_begin (change nothing)

// ---- profc mirror (PROFC_NODE, reference src/profc.h:9-13), timed on the GPU timeline -----------------------------------------
int prof_scope_id(smg_hierarchy* h, const char* name);
hipEvent_t prof_event(smg_hierarchy* h);
void prof_collect(smg_hierarchy* h);
struct ProfGuard {
    smg_hierarchy* h; int idx = -1;
    ProfGuard(smg_hierarchy* hh, const char* name) : h(hh)
    {
        if (!h->prof_on) return;
        ProfRec r; r.scope = prof_scope_id(h, name); r.e0 = prof_event(h); r.e1 = prof_event(h);
        (void)hipEventRecord(r.e0, h->stream);
        h->recs.push_back(r);
        idx = (int)h->recs.size() - 1;
    }
    ~ProfGuard() { if (idx >= 0) (void)hipEventRecord(h->recs[idx].e1, h->stream); }
};

// ---- container helpers -----------------------------------------------------------------------------------------------------------
// CSR/CSC array sanity: monotone pointers, indices in range.  Returns an error string or nullptr.
const char* check_compressed(int n_major, int n_minor, const int* ptr, const int* idx);
int set_prolong(smg_hierarchy* h, int lv, Csr&& P);   // mg[lv].P = PT^T = P_full = P  (reference src/mg_precompute.cpp:74-76)
Mesh wrap_mesh(const double* V, int nV, const int* F, int nF);
// what the handle holds in HBM, by purpose: the non-zero (name, bytes) entries that smg_debug_device_bytes prints and totals
std::vector<std::pair<std::string, long long>> device_byte_entries(const smg_hierarchy* h);

// ---- precompute (smg_precompute.cpp) ------------------------------------------------------------------------------------------------
int spectral_bounds(smg_hierarchy* h);          // Gershgorin bounds of D^-1 A on every smoothed level (Chebyshev-Jacobi)
int ensure_spectral_bounds(smg_hierarchy* h);   // ... only when a level is smoothed that way and the values changed
int refresh_host_values(smg_hierarchy* h);      // host copies of mg[l].A after a device-side value-only re-precompute
int ensure_P_int(smg_hierarchy* h, int lv);     // ... and P / PT of the level
int ensure_A_int(smg_hierarchy* h, int lv);     // the level matrix in the internal numbering on the host (built on demand where the device filled the panels)

// ---- independent meshes in one handle (smg_union.cpp) ---------------------------------------------------------------------------------
int union_coarse_factor(smg_hierarchy* h, const double* d_vals, bool first);   // the members' dense inverses, side by side (first: + the bookkeeping)
int union_begin_solve(smg_hierarchy* h, int k);                                // per-member solve state

// ---- cycle (smg_cycle.cpp) -----------------------------------------------------------------------------------------------------------
enum { LV_GS = 0, LV_JACOBI = 1, LV_CHEBY = 2 };
int level_kind(const smg_hierarchy* h, int lv);   // the smoother of a level under the handle's selection
inline bool level_is_jacobi(const smg_hierarchy* h, int lv) { return level_kind(h, lv) != LV_GS; }   // needs the second iterate buffer

// what of a level's first pre-smoothing sweep exists when its V-cycle starts
enum { FIRST_NONE = 0,
       FIRST_LAUNCH = 1,   // its first launch, produced by the restriction launch of the finer level (FirstColour): the first colour
                           // (Gauss-Seidel, in Lv.u) or the whole first sweep / step (Jacobi / Chebyshev, in Lv.t)
       FIRST_SWEEP = 2 };  // level 0 inside an outer iteration: the whole first sweep / step, produced out of place into Lv.t by the
                           // launches that also formed the outer residual (enqueue_head)

int ensure_work(smg_hierarchy* h, int k);         // the level vectors (and sweep plans, spectral bounds) for k internal columns
int ensure_fp32(smg_hierarchy* h, int k);         // ... and the fp32 images and vectors of the mixed-precision cycle
// one V-cycle on level 0 with the handle's sweeps and precision: L0.u = V(L0.b, L0.u) (precision 1: the same on vecs<float>(L0)); first: FIRST_* of the fp64 cycle
int enqueue_vcycle(smg_hierarchy* h, int k, const Ctrl* ctrl, int first);
int enqueue_residual_ss(smg_hierarchy* h, int k, bool fuse_decide = false, double* sumsq_out = nullptr);   // |RHS_u - A_0 z_u|^2 (+ break test), head-fused or not
int enqueue_cycle_part(smg_hierarchy* h, int k, const double* d_sumsq);                                     // (break test on *d_sumsq,) the cycle of an outer iteration
int apply_A(smg_hierarchy* h, int lv, SellMode mode, const double* x, const double* b, double* y, int k, const Ctrl* ctrl);   // SELL_AX / SELL_RESID with the level's matrix
bool head_fusable(smg_hierarchy* h, int k);
int internal_cols(const smg_hierarchy* h, int k);
int coarse_stall_check(smg_hierarchy* h);

template <typename Fn>
static int capture_graph(smg_hierarchy* h, hipGraphExec_t* out, Fn&& body)
{
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    int rc = body();
    hipError_t e = hipStreamEndCapture(h->stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fail(SMG_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail(SMG_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    return SMG_OK;
}

// ---- solve bookkeeping (smg_solve.cpp) ------------------------------------------------------------------------------------------------
int latch_solve_opts(smg_hierarchy* h, const smg_solve_opts& o);   // the (checked) options become the handle's selection
int reset_ctrl(smg_hierarchy* h, int cap);                         // a fresh control block on the stream: not done, the handle's tol, room for `cap` history entries

// ---- Gauss-Seidel sweep plans (smg_sweep_plans.cpp) -------------------------------------------------------------------------------
// How relax(sweeps) runs on a Gauss-Seidel level: at most one plan is set; none: one launch per colour.
struct SweepPlan {
    const TiledDev* tiled = nullptr;   // overlapped tiling: one out-of-place launch (smg_tiled.hpp)
    const WgsBuf* wave = nullptr;      // wave Gauss-Seidel: one launch per piece colour (smg_wgs.hpp)
    const BgsBuf* block = nullptr;     // block Gauss-Seidel: one launch per block colour (smg_bgs.hpp)
    bool colours() const { return !tiled && !wave && !block; }
};
// level lv, k columns, fp64 or fp32 cycle, `first` (FIRST_*): the plan its relax(sweeps) runs with (built plans only: prepare_sweep_plans)
SweepPlan sweep_plan(const smg_hierarchy* h, int lv, int k, int sweeps, bool fp64, int first);
int prepare_sweep_plans(smg_hierarchy* h, int k, int sa, int sb);   // plans + second iterate for relax(sa) / relax(sb) (never inside a graph capture)
// the sweep plans a small level would want for a default solve (one column, the handle's pre / post sweeps), built ahead of the first solve
int prepare_level_plans(smg_hierarchy* h, int lv);
int refresh_plan_values(smg_hierarchy* h);      // the plans hold copies of the level values (value-only re-precompute)
void drop_sweep_plans(smg_hierarchy* h);        // ... and describe one matrix image: dropped when the images are rebuilt

}  // namespace smg
