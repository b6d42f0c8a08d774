/*
 * smg.h -- C ABI of libsmg: the MI355X-native surface-multigrid solve path.
 *
 * Drop-in boundary for the `mg_VCycle` / `min_quad_with_fixed_mg_*` path of
 * HTDerekLiu/surface_multigrid_code.  The reference has no FFI layer: its boundary is the set of C++
 * free functions in src/min_quad_with_fixed_mg.h:32-113, src/mg_VCycle.h:22-76 and
 * src/mg_precompute.h:15-32 taking Eigen objects by reference.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference checkout).  The C++ mirror with the
 * reference's own function names/argument order lives in surface_multigrid_code_amd/csrc/mg_api.hpp;
 * INTEGRATION.md shows the Eigen-side binding.
 *
 * Conventions
 *   - plain pointers and sizes only; fp64 values, int32 indices (Eigen's default StorageIndex);
 *   - sparse matrices are passed as CSR (rowptr, col, val).  For the symmetric system matrix these are the
 *     very arrays Eigen's column-major SparseMatrix holds (outerIndexPtr, innerIndexPtr, valuePtr); for the
 *     prolongation P a `_csc` twin takes Eigen's compressed-column arrays directly;
 *   - dense blocks are column-major n x k with a leading dimension, exactly Eigen::MatrixXd / VectorXd;
 *   - every function returns an int status: 0 = ok, < 0 = error (enum below); nothing throws across the ABI;
 *     `smg_last_error()` gives a thread-local message;
 *   - a handle owns its device memory and one HIP stream; a handle is not thread-safe, distinct handles are;
 *   - compute entry points REQUIRE a HIP device: without one they fail with SMG_ERR_NO_DEVICE -- there is no
 *     CPU fallback inside this library (the CPU oracle lives in oracle/ and is test infrastructure only).
 */
#ifndef SMG_H
#define SMG_H

#ifdef __cplusplus
extern "C" {
#endif

#define SMG_VERSION 553

enum {
    SMG_OK = 0,
    SMG_ERR_INVALID = -1,     /* bad argument / call order */
    SMG_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    SMG_ERR_HIP = -3,         /* a HIP runtime call failed */
    SMG_ERR_NONFINITE = -4,   /* residual became NaN/Inf */
    SMG_ERR_ALLOC = -5,
    SMG_ERR_IO = -6,
    SMG_ERR_REDUCE = -7       /* the caller's reduction (smg_solve_sharded) reported a failure */
};

enum { SMG_HOST = 0, SMG_DEVICE = 1 };         /* where the dense blocks handed to smg_solve live */

/* decimation types of mg_precompute (src/mg_precompute.h:9: 0 qslim, 1 midpoint, 2 vertex removal) */
enum { SMG_DEC_QSLIM = 0, SMG_DEC_MIDPOINT = 1, SMG_DEC_VERTEX_REMOVAL = 2 };

/* smoother of the V-cycle (the slot of relax(), src/mg_VCycle.cpp:113-178).  The reference only has Gauss-Seidel; damped Jacobi is
 * the "Gauss-Seidel/Jacobi smoothing" of this build's brief: one whole-matrix launch per sweep instead of one launch per colour.
 *   GS      forward Gauss-Seidel on every level: the reference's sweep on the colour-major numbering (default)
 *   JACOBI  damped Jacobi on every level:  u_i <- u_i + omega * ((b_i - sum_{j != i} A(j,i) u_j) / A_diag_i - u_i), all rows from the old u
 *   HYBRID  Gauss-Seidel on the levels with more than `jacobi_max_rows` unknowns (bandwidth-bound: a sweep costs its bytes),
 *           Jacobi on the smaller ones (launch-latency-bound: a sweep costs its launches)
 *   CHEBYSHEV / HYBRID_CHEBYSHEV  the same two layouts with Chebyshev-accelerated Jacobi instead of damped Jacobi: relax(iters) is ONE
 *           polynomial of degree iters + 1 in D^-1 A (so V(2,2) smooths with degree 3: three whole-matrix launches where two Gauss-Seidel
 *           sweeps take two launches per colour), optimal on [cheby_fraction * lam, lam] with lam the Gershgorin bound
 *           max_i sum_j |A(j,i)| / A_diag_i.  Step s of the three-term recurrence (theta, delta = centre / half width of that interval,
 *           sigma = theta / delta, rho_0 = 1 / sigma):   r_i = (b_i - sum_{j != i} A(j,i) u_j) / A_diag_i - u_i,
 *           s = 0: d = r / theta;  s >= 1: rho_s = 1 / (2 sigma - rho_{s-1}), d = rho_s rho_{s-1} d + (2 rho_s / delta) r;   u += d.
 *           Measured: as many cycles as Gauss-Seidel everywhere where damped Jacobi needs 30-70 % more (anisotropic torus, C5). */
enum { SMG_SMOOTH_GS = 0, SMG_SMOOTH_JACOBI = 1, SMG_SMOOTH_HYBRID = 2, SMG_SMOOTH_CHEBYSHEV = 3, SMG_SMOOTH_HYBRID_CHEBYSHEV = 4 };

typedef struct smg_hierarchy smg_hierarchy;

/* Parameters the reference hard-codes or passes through default-argument overloads:
 *   tol = 1e-3 (min_quad_with_fixed_mg.cpp:63,270), max_iter = 20 (:77,:285), pre = post = 2 (:102-103,:324-325) */
typedef struct {
    double tol;
    int max_iter;
    int pre, post;
    int verbosity;     /* 0 silent; 1 prints "MG iteration: i, residual: r" lines like the reference (:111) */
    int check_every;   /* smg_solve looks at the device-side convergence flag every this many iterations; 0 (default): adaptive -- the
                          number of cycles still needed is extrapolated from the last two residuals, and all but the last of them are
                          enqueued before the next look.  Results do not depend on it (the break test runs on the device). */
    int use_graph;     /* 1: replay one captured hipGraph per outer iteration; 0: eager launches */
    int precision;     /* 0 (default): everything fp64, the reference arithmetic.  1: mixed -- the outer iterate and the
                          residual (hence r_his and the stopping test) stay fp64, the V-cycle runs on fp32 copies of the
                          operators as z += V32(RHS - A z): same iteration in exact arithmetic, fp64 accuracy at convergence,
                          ~2/3 of the bytes (BASELINE config 5: fp32 vs fp64) */
    int smoother;      /* SMG_SMOOTH_GS (default, the reference) / SMG_SMOOTH_JACOBI / SMG_SMOOTH_HYBRID */
    double omega;      /* Jacobi damping factor (default 0.8) */
    int jacobi_max_rows; /* HYBRID*: levels with at most this many unknowns are smoothed by (Chebyshev-)Jacobi (default 100000) */
    double cheby_fraction; /* lower end of the Chebyshev interval as a fraction of the Gershgorin bound (default 0.1) */
} smg_solve_opts;
void smg_solve_opts_default(smg_solve_opts *o);

int smg_version(void);
const char *smg_last_error(void);
int smg_device_count(void);
/* device memory currently held by all libsmg handles / assemblers of this process, in bytes (memory budget reporting) */
long long smg_device_bytes_live(void);
/* what ONE handle holds in HBM, by purpose: lines "name bytes" (and "total bytes") written into buf (memory budget reporting) */
int smg_debug_device_bytes(const smg_hierarchy *h, char *buf, int cap);

/* ---- std::vector<mg_data> (src/mg_data.h:11-27) ---------------------------------------------------------------- */
/* mg.reserve(nLvs) */
smg_hierarchy *smg_hierarchy_create(int n_levels);
void smg_hierarchy_destroy(smg_hierarchy *h);
int smg_hierarchy_levels(const smg_hierarchy *h);
/* Use an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream) instead of the handle's own. */
int smg_hierarchy_set_stream(smg_hierarchy *h, void *hip_stream);
/* Smoother used by smg_vcycle / smg_relax and the raw / bench entry points (which take no smg_solve_opts); smg_solve* set the same
 * state from their opts.  omega <= 0 keeps the current value, jacobi_max_rows < 0 likewise. */
int smg_hierarchy_set_smoother(smg_hierarchy *h, int smoother, double omega, int jacobi_max_rows);
int smg_hierarchy_set_chebyshev(smg_hierarchy *h, double cheby_fraction);     /* (0, 1); <= 0 keeps the current value */
/* the Gershgorin bound the Chebyshev smoother of level lv uses (0 before smg_precompute / on the coarsest level) */
double smg_level_spectral_bound(const smg_hierarchy *h, int lv);
/* mg[lv].P_full = mg[lv].P = P; mg[lv].PT = P^T  (what mg_precompute stores per level, src/mg_precompute.cpp:71-77).
 * P is #V_{lv-1} x #V_lv for lv = 1 .. n_levels-1 (the operator lives on the COARSER level, mg_VCycle.cpp:80,:91). */
int smg_level_set_prolong(smg_hierarchy *h, int lv, int n_fine, int n_coarse, const int *rowptr, const int *col,
                          const double *val);
int smg_level_set_prolong_csc(smg_hierarchy *h, int lv, int n_fine, int n_coarse, const int *colptr,
                              const int *rowidx, const double *val);
/* mg[lv].V / mg[lv].F (optional; not used by the solve) */
int smg_level_set_mesh(smg_hierarchy *h, int lv, const double *V, int nV, const int *F, int nF);
/* read them back (query sizes with NULL arrays first); V: nV x 3 row-major, F: nF x 3 */
int smg_level_get_mesh(const smg_hierarchy *h, int lv, int *nV, int *nF, double *V, int *F);

/* ---- mg_precompute (src/mg_precompute.h:26-32, src/mg_precompute.cpp:15-87) ------------------------------------ */
/* Builds the hierarchy from a triangle mesh: level count by the reference's float rule (:27-38), per level
 * tarF = round(#F * ratio) (:59), edge-collapse decimation + prolongation.  V: nV x 3 row-major, F: nF x 3.
 * dec_type (src/mg_precompute.cpp:10): 0 qslim (quadric error metric, merged vertex at the quadric's minimiser), 1 mid-point
 * (shortest edge first), 2 vertex removal (shortest edge first, merged vertex on an end point).
 * libsmg's own host implementation of the reference's construction (src/SSP_midpoint.cpp, src/SSP_collapse_edge.cpp, src/joint_lscm.cpp,
 * src/query_fine_to_coarse.cpp): boundary closed by a vertex at infinity, greedy shortest-edge collapse to the mid-point with libigl's
 * refuse / re-cost queue discipline, joint conformal flattening of the 1-rings before / after every collapse in the reference's three
 * cases (interior, one boundary end point, boundary edge with its snap candidates), the reference's validity and quality thresholds;
 * same P structure (3 stored entries per row, rows sum to 1).  Written from the formulation on own data structures; reproduces the
 * reference's checked-in 08_subdiv_remesh outputs point for point (tests/golden/bunny_remesh_500.npz).  Ties between exactly
 * equal-cost edges may be broken differently than libigl's edge numbering does (csrc/smg_decimate.cpp).
 * ONLY dec_type 1 (mid-point, the default of every reference caller: src/mg_precompute.cpp:94, 03_mg_solver/main.cpp:37) restates the reference and is
 * pinned against its outputs.  dec_type 0 and 2 run the same collapse machinery with LIBSMG'S OWN cost and placement (quadric error / end-point placement as
 * described above): they are NOT restatements of src/SSP_qslim.cpp / src/SSP_vertexRemoval.cpp and no parity with them is claimed. */
int smg_mg_precompute(const double *V, int nV, const int *F, int nF, float ratio, int nVCoarsest, int dec_type,
                      smg_hierarchy **out);
/* The same with an opt-in departure from the reference's plain greedy collapse order: a surviving vertex may stand for at most
 * absorption_cap x (#F / tarF) input vertices (edges that would exceed that wait; the bound doubles when nothing else can be collapsed).
 * Shortest-edge-first decimation coarsens densely sampled regions far beyond the requested ratio before it touches the rest, which the
 * V-cycle pays for (ogre.obj: factor 0.6 -> 0.3 with a cap of 2).  absorption_cap = 0 is smg_mg_precompute. */
int smg_mg_precompute_capped(const double *V, int nV, const int *F, int nF, float ratio, int nVCoarsest, int dec_type,
                             float absorption_cap, smg_hierarchy **out);
/* The same, keeping the record of every collapse (the reference's decInfo / decIM outputs of SSP_decimate, src/SSP_decimate.h:10-22;
 * host memory ~0.5 kB per collapse) when keep_log != 0: smg_query_coarse_to_fine needs it. */
int smg_mg_precompute_logged(const double *V, int nV, const int *F, int nF, float ratio, int nVCoarsest, int dec_type,
                             float absorption_cap, int keep_log, smg_hierarchy **out);
/* query_coarse_to_fine (src/query_coarse_to_fine.h; 08_subdiv_remesh/main.cpp:146): n points on the mesh of level lv (lv >= 1) --
 * face[i] a face of mg[lv].F, bary[3i..3i+2] barycentric coordinates with respect to its corners -- are carried through the bijection
 * of the successive self-parameterisation onto the mesh of level lv - 1 by undoing the collapses of that coarsening step, last to
 * first: out_face[i] a face of mg[lv-1].F, out_bary[3i..] coordinates there (>= 0, sum 1).  The level must have been built by
 * smg_mg_precompute_logged(keep_log = 1); SMG_ERR_INVALID otherwise (also after smg_hierarchy_load: the record is not part of the
 * .smgh file).  Host only (no GPU involved). */
int smg_query_coarse_to_fine(const smg_hierarchy *h, int lv, int n, const int *face, const double *bary, int *out_face,
                             double *out_bary);
/* query_fine_to_coarse (src/query_fine_to_coarse.h; what get_prolong does for the vertices, src/get_prolong.cpp:23-57): the other
 * direction -- points of level lv - 1's mesh onto level lv's mesh, collapses first to last.  A vertex of the fine mesh (one-hot
 * coordinates in any of its faces) arrives where its row of mg[lv].P_full says. */
int smg_query_fine_to_coarse(const smg_hierarchy *h, int lv, int n, const int *face, const double *bary, int *out_face,
                             double *out_bary);
/* Hierarchy of a mid-point-subdivided mesh: the n_sub finest transfer operators are the subdivision operators
 * (09_random_subdiv_remesh/main.cpp:46-140), levels below the base mesh come from smg_mg_precompute's decimator
 * (ratio, nVCoarsest applied to the base mesh; pass n_extra_levels = -1 for the float rule).  Outputs the fine
 * mesh through V_out/F_out (caller-allocated: nV_fine x 3, nF * 4^n_sub x 3) when non-null. */
int smg_mg_precompute_subdiv(const double *V, int nV, const int *F, int nF, int n_sub, float ratio, int nVCoarsest,
                             int n_extra_levels, smg_hierarchy **out, double *V_out, int *F_out);

/* mg_precompute_block (src/mg_precompute_block.h, src/mg_precompute_block.cpp:23-95; get_prolong_block,
 * src/get_prolong.cpp:59-115): same hierarchy with P (x) I_3 for 3-DOF-per-vertex systems, DOF index = 3*vertex + d.
 * To the V-cycle the block system is a plain sparse matrix. */
int smg_mg_precompute_block(const double *V, int nV, const int *F, int nF, float ratio, int nVCoarsest, int dec_type,
                            smg_hierarchy **out);
/* Block (3 x 3) kernels for such hierarchies.  The reference runs its scalar kernels on the 3n x 3n system its caller assembles
 * (06_example_balloon_sim/sim_utils/implicit_euler_mg_balloon.h:63-76: an elasticity Hessian, one 3 x 3 block per vertex pair).
 * smg_precompute recognises the structure -- every prolongation of the form Pv (x) I_3 (however the handle got them: this builder,
 * smg_level_set_prolong, a file), no constraints, n % 3 == 0 -- and then keeps the level matrices in 3 x 3 blocks (76 instead of
 * 108 bytes per block), numbers VERTICES colour-major and lets one lane update the three DOFs 3v, 3v+1, 3v+2 of its vertex in order:
 * the reference's lexicographic Gauss-Seidel sweep (src/mg_VCycle.cpp:146-160) on that numbering, with as many launches per sweep as
 * the vertex graph has colours; P (x) I_3 is applied from Pv.  Results: the reference algorithm on the scalar matrix, bit for bit
 * per kernel in the device numbering (smg_level_get_matrix(..., internal = 1) is the scalar matrix in it).
 * mode: -1 (default) decide at smg_precompute: structure present AND the blocks of A at least half full (kron(S, I_3) is better
 * served as three right-hand sides of a scalar problem); 0 never; 3 required (smg_precompute fails when the structure is absent).
 * Constraints: pinned VERTICES (all three DOFs 3v, 3v+1, 3v+2 in `known`) keep the structure -- the reference's slices and column drops
 * (src/min_quad_with_fixed_mg.cpp:137-257) are formed on the scalar matrices and factor as Pv' (x) I_3 again -- and stay on the block
 * kernels; constraints on single degrees of freedom select the scalar path (mode 3: smg_precompute fails and says so).
 * The mixed-precision cycle (smg_solve_opts.precision) is available: the V-cycle runs on an fp32 image of the 3 x 3-block panels. */
int smg_hierarchy_set_block_mode(smg_hierarchy *h, int mode);
int smg_hierarchy_block_size(const smg_hierarchy *h);   /* 1 or 3: what the last smg_precompute decided */
/* block image of A_lv (lv < n_levels - 1, block hierarchies only): stored 3 x 3 blocks, allocated block slots (SELL padding
 * included), vertex colours = launches per Gauss-Seidel sweep */
int smg_level_block_stats(const smg_hierarchy *h, int lv, long *n_blocks, long *n_block_slots, int *n_vertex_colors);
/* The block SELL image of A_lv as the device holds it (tests; built on the host, works without a GPU once the host half of
 * smg_precompute has run on a block hierarchy).  Slices of <= 64 vertices, one lane per vertex; panel column j of slice s: block column
 * col[(slice_off[s] + j) * 64 + lane] (-1 = padding) and value plane e = 3 * row_in_block + col_in_block at
 * val[((slice_off[s] + j) * 9 + e) * 64 + lane].  Query n_slices / n_panel_cols with NULL arrays first. */
int smg_level_get_block_image(const smg_hierarchy *h, int lv, int *n_slices, int *n_panel_cols, int *slice_row, int *slice_off, int *slice_w,
                              int *col, double *val);
/* relax() with MANY right-hand sides (reference k > 1 branch, src/mg_VCycle.cpp:161-177: k independent lexicographic sweeps).
 * With k a multiple of 16 (k >= 16) the levels of at least min_rows rows (default: never; SMG_BGS_MIN_ROWS; < 0: never; SMG_BGS=0: never)
 * can sweep BLOCK-wise: the level is cut into compact blocks of <= 64 rows, blocks are coloured, one launch per block colour; a wavefront
 * owns (block, 16 columns), reads the block's rows and its rim once into LDS and updates the block's rows there, <= 16 independent rows at a time.  That is the reference's lexicographic sweep on the numbering (block colour, block, vertex colour, row) -- per kernel bit for bit
 * what the oracle computes on that numbering, smg_level_get_block_gs_order -- and reads the iterate ~1.65 times per sweep instead of 3
 * (the multi-colour order of the wide kernels re-reads it once per colour).  Measured at 1 M rows: the fine-level sweep 8 - 10 % faster at
 * 64 columns, 22 % at 32; the plan costs a graph partition of the level at the first such solve, so it is an option for
 * callers that solve often, not the default.  It is a different, equally valid Gauss-Seidel order than the multi-colour one: iterates of
 * the two paths differ, converged solutions agree to the tolerance (same cycle counts measured).  The outer residual is then a launch of
 * its own (the multi-colour path folds it into its first sweep).  Changing min_rows takes effect at the next solve. */
int smg_hierarchy_set_block_gs(smg_hierarchy *h, int min_rows);
/* The block-sequential order of level lv as a solve with k columns would use it (after smg_precompute; builds the plan): *n_blocks,
 * *n_colors, color_ptr[n_colors + 1] (blocks per block colour), blk_ptr[n_blocks + 1] (positions per block), rows[n] (position -> row
 * in the INTERNAL numbering, smg_level_get_perm), stats[2] = {rows gathered per row beyond the iterate itself, share of the walk's row
 * slots that hold a row of their own (the rest repeat one)}.  Any pointer may be NULL.  Returns 1 when level lv sweeps block-sequentially for this k, 0 when
 * it does not (nothing is written then), < 0 on error. */
int smg_level_get_block_gs_order(smg_hierarchy *h, int lv, int k, int *n_blocks, int *n_colors, int *color_ptr, int *blk_ptr, int *rows, double *stats);
/* relax() on the Galerkin levels of the REFERENCE's own hierarchies (smg_mg_precompute = src/mg_precompute.cpp:15-87: A_l = PT A P with 18 - 30 entries
 * per row, 11 - 15 colours).  Such a level sweeps PIECE-wise: compact pieces of <= 64 rows, the piece graph coloured (4 - 6 colours whatever the rows'
 * degree), one launch per piece colour, one wavefront per piece (lane = row, the row in registers, the piece's rows and rim in LDS, rows updated phase by
 * phase there).  That is the reference's lexicographic sweep (src/mg_VCycle.cpp:146-160) on the numbering (piece colour, piece, local colour, row) -- per
 * kernel bit for bit what the oracle computes on that numbering, smg_level_get_wave_gs_order.  A different, equally valid Gauss-Seidel order than the
 * multi-colour one: iterates differ, converged solutions agree to the tolerance, cycle counts are the same (measured).
 * mode: -1 (default) automatic = Gauss-Seidel levels of 512 - 600 000 rows with more than 5 colours or rows of more than 12 entries that have no
 * one-launch relax() (overlapped tiling), any number of columns (the order of a level's sweep never depends on k: a column-sharded solve iterates bit for bit
 * like the fused one), fp64 cycles; 0 never (one launch per colour); 1 every Gauss-Seidel level in that size range, for every k (such a level then takes no
 * one-launch relax() either: that exists for k <= 7 only, and the order must not depend on k).
 * SMG_WGS=0 / 1 / 2 overrides (off / automatic / every level).  Takes effect at the next solve. */
int smg_hierarchy_set_wave_gs(smg_hierarchy *h, int mode);
/* Memory against speed (the reference has no counterpart: mg_data holds Eigen's compact CSC, src/mg_data.h:11-27).  By default every operator's SELL panels get a
 * FIXED pitch -- room for the level's widest slice (A_0 of a triangle mesh: 12 columns for 7 used) -- so that a wave addresses its panel from its slice number alone
 * and no launch waits for a table: 545 MB for the 171 MB of CSR operators of the 1 M-vertex benchmark hierarchy.  on = 1: compact panels + a slice-offset table
 * (what matrices with a few very wide slices get anyway): 421 MB there, the V(2,2) cycle 14 - 16 % slower (0.313 -> 0.362 ms: one more dependent load in front of
 * every launch), results bit-identical.  For many resident meshes per GPU.  Takes effect at the next smg_precompute, which is then a full one. */
int smg_hierarchy_set_memory_lean(smg_hierarchy *h, int on);
/* The piece-sequential order of level lv as a solve with k columns would use it (after smg_precompute; builds the plan): *n_pieces, *n_colors,
 * color_ptr[n_colors + 1] (pieces per piece colour), piece_ptr[n_pieces + 1] (positions per piece), rows[n] (position -> row in the INTERNAL numbering,
 * smg_level_get_perm), stats[3] = {rows gathered per row beyond the iterate itself, mean phases per piece, most phases of a piece}.  Any pointer may be
 * NULL.  Returns 1 when level lv sweeps piece-wise for this k, 0 when it does not (nothing is written then), < 0 on error. */
int smg_level_get_wave_gs_order(smg_hierarchy *h, int lv, int k, int *n_pieces, int *n_colors, int *color_ptr, int *piece_ptr, int *rows, double *stats);
/* ---- independent meshes in ONE handle (BASELINE north_star: "independent RHS columns / independent meshes shard") ----------------------------------
 * Across GPUs: one handle per device.  On ONE GPU separate handles do not overlap (a hipGraphLaunch of ~50 kernel nodes is enqueued under a process-wide
 * lock), so many small meshes go into one block-diagonal handle whose every launch serves all of them.
 * smg_hierarchy_create_union: members = m hierarchies with their prolongations set (smg_mg_precompute, smg_level_set_prolong, ...; same number of levels,
 * scalar); *out gets P_full_l = diag(P_full_l of the members), rows and columns in member order.  The members are only read and may be destroyed afterwards.
 * smg_precompute(out, A, ...) then takes the block-diagonal system (member i's rows are [first, first + count) of smg_union_member_rows; constraints in
 * that numbering).  What the reference does PER MESH stays per mesh: every member is its own min_quad_with_fixed_mg_solve loop
 * (src/min_quad_with_fixed_mg.cpp:105-134) -- its own residual norm, history and break test; a member whose test has passed keeps the iterate it had then
 * while the others go on (smg_union_get_history after smg_solve / smg_solve_end: its residual history, and the reference's return value for it) -- and
 * coarseSolve() uses the members' OWN dense inverses (sum n_i^2 entries, not (sum n_i)^2; every member's coarsest level must lie in the dense range).
 * The handle's own r_his is the norm over all members, `converged` = every member's loop ended below the tolerance.  Members are numerically isolated:
 * one whose residual stops being finite ends ITS loop as failed (its history ends with that value, its `converged` is 0, the handle's too) while the
 * others iterate on to their own tolerance, unaffected bit for bit; it no longer enters the handle's norm.  fp64 cycles only (precision = 1 is refused
 * before anything of the handle changes); no split-phase /
 * sharded iteration on a union.  Numberings and sweep orders are those of the union's matrices: a member's iterates agree with a stand-alone solve of the
 * same mesh to the tolerance, not bit for bit. */
int smg_hierarchy_create_union(const smg_hierarchy *const *members, int m, smg_hierarchy **out);
int smg_union_members(const smg_hierarchy *h);                                           /* 0: not a union */
int smg_union_member_rows(const smg_hierarchy *h, int member, int *first, int *count);   /* member's rows in the caller's numbering of level 0 */
int smg_union_get_history(smg_hierarchy *h, int member, double *r_his, int cap, int *n_his, int *converged);
/* The coarsest level's solver (coarseSolve(), src/mg_VCycle.cpp:181-201; solver.compute(Ac), src/min_quad_with_fixed_mg.cpp:47-48, :253-254).  Three of them,
 * chosen by size and by what the caller does (all: <= 1e-11 from LDL^T, deterministic):
 *  - DENSE INVERSE, up to n_max unknowns (smg_hierarchy_set_coarse_dense_max, default 16384, or SMG_COARSE_DENSE_MAX): the matrix is inverted on the device
 *    (blocked symmetric Gauss-Jordan on the matrix cores) and applied as a bandwidth-bound product (8 n^2 bytes of HBM, half of them streamed per cycle and
 *    column): 0.02 ms per cycle at 4 k unknowns, 0.2 ms at 16 k; the cheapest to apply below ~6 k unknowns, n^3 flops to build (2.4 ms at 4 k, 0.1 s at 16 k).
 *  - SCHUR COMPLEMENT (smg_hierarchy_set_coarse_schur below): one level of exact block elimination, only the separator (0.27 - 0.43 n rows) inverted densely.
 *  - SPARSE CHOLESKY P A P^T = L L^T -- what the reference's Eigen::SimplicialLDLT does -- computed on the host during smg_precompute (nested-dissection
 *    order), the two triangular solves on the device (one launch each, rows wait for the rows they read): O(n log n) memory, 2.6 ms per solve at 16 k
 *    unknowns, 16 ms at 63 k; for coarsest levels beyond the other two, or on request.  Not available with it: the mixed-precision cycle.
 * So mg_precompute's nVCoarsest may be anything the reference accepts, down to a 1-level call on the whole mesh.
 * smg_hierarchy_coarse_solver: 0 dense inverse / 1 sparse Cholesky / 2 Schur complement after a precompute; *factor_entries: n^2, the entries of L, resp. the
 * doubles the Schur solver keeps. */
int smg_hierarchy_set_coarse_dense_max(smg_hierarchy *h, int n_max);
int smg_hierarchy_coarse_solver(const smg_hierarchy *h, long *factor_entries);
/* The Schur-complement coarse solver (csrc/smg_schur.hpp): the rows are cut into compact blocks of <= 64, a vertex cover of the entries between blocks becomes
 * the separator, every block is inverted in LDS, and only the separator's Schur complement is inverted densely.  coarseSolve becomes g = b_S - sum W_i^T b_i,
 * x_S = S^-1 g, x_i = D_i^-1 b_i - W_i x_S: three launches instead of two, a quarter of the bytes (or less).  Same answer to rounding, bit-identical from
 * run to run; available in fp32 for the mixed-precision cycle.  For coarsest levels of n_min (default 2048, or SMG_COARSE_SCHUR_MIN; n_min < 0: unchanged)
 * to 65 536 (SMG_COARSE_SCHUR_MAX) unknowns:
 *   when = 0  never;
 *   when = 1  from the first smg_precompute on;
 *   when = 2  (default, or SMG_COARSE_SCHUR) THE CHOICE BY COST:
 *             - below 6 144 unknowns (SMG_COARSE_SCHUR_BIG) a handle that is factored once keeps the dense inverse (its cycle is ~4 us cheaper at 4 k unknowns);
 *               the first VALUE-ONLY re-precompute moves it to the Schur complement -- a caller that sends new values for an old pattern (05_example_mean_
 *               curvature_flow/main.cpp:74, 06: implicit_euler_mg_balloon.h:75) pays the factorisation at every step: 0.9 ms instead of 2.4 at 3 952 unknowns,
 *               value-only smg_precompute 3.1 -> 1.4 ms (the switch itself costs one plan on the host, ~ms, once);
 *             - from 6 144 unknowns on it is cheaper to build AND to apply: taken at the first precompute (15 804 unknowns: 38 us per solve and 182 MB
 *               against 204 us and 2 GB);
 *             - above the DEFAULT n_max (16 384) it stands in for the sparse factorisation (63 210 unknowns: 0.30 ms per solve against 15.8 ms, 2.6 GB
 *               against 0.1 GB).  A caller who SET n_max (smg_hierarchy_set_coarse_dense_max, SMG_COARSE_DENSE_MAX) gets the sparse factorisation above it --
 *               that call bounds memory, and the separator's inverse is dense -- unless when = 1 asks for the Schur solver explicitly.
 * A matrix whose blocks touch more than 128 separator rows each, or whose separator exceeds 0.7 n or 24 576 rows (its inverse is dense), or whose arena
 * would exceed SMG_SCHUR_ARENA_MAX_MB (default 6 144) or does not fit the device, keeps the dense inverse resp. the sparse factorisation (nothing half-built
 * stays behind).  After every factorisation the diagonals of the inverted blocks and of S^-1 are checked: a coarsest matrix that is not positive definite
 * fails smg_precompute with SMG_ERR_INVALID, as the sparse factorisation does. */
int smg_hierarchy_set_coarse_schur(smg_hierarchy *h, int when, int n_min);
/* On-disk hierarchy ({P_full_l}, optional V/F per level): build the expensive hierarchy once, ship it as a fixture.
 * Format (little endian): "SMGH" u32 version=1 i32 n_levels, then per level: i32 nV i32 nF f64 V[3nV] i32 F[3nF],
 * and for lv >= 1: i32 n_rows i32 n_cols i32 nnz i32 ptr[n_rows+1] i32 col[nnz] f64 val[nnz]. */
int smg_hierarchy_save(const smg_hierarchy *h, const char *path);
int smg_hierarchy_load(const char *path, smg_hierarchy **out);

/* ---- min_quad_with_fixed_mg_precompute (src/min_quad_with_fixed_mg.h:32-36 and :72-77) ------------------------- */
/* A: n x n symmetric, CSR == CSC.  known == NULL / n_known == 0 selects the no-constraint overload
 * (.cpp:3-51); otherwise the `known` overload (.cpp:137-257): unknown = setdiff, LHS/Auk slices, P re-organised
 * to unknowns with the all-(<=1e-15) column drop cascade, Galerkin A_l = PT_l A_{l-1} P_l, +1e-12 on the coarsest
 * diagonal, A_diag, coarsest factorisation (here: dense inverse computed on the device).  May be called again on
 * the same handle (new matrix every time step, 05_example_mean_curvature_flow/main.cpp:74); always restarts
 * from P_full.
 * A first (pattern-changing) call works on several host threads: the sparse algebra and the numberings on a thread of its own and a
 * process-wide pool of SMG_HOST_THREADS workers (default min(hardware threads, 32), kept for later calls), while the calling thread
 * brings the device up and builds the level images as they become ready -- 0.1 s for a million unknowns.  The arrays are read until
 * the call returns and not after; errors are reported on the calling thread as usual. */
int smg_precompute(smg_hierarchy *h, int n, const int *rowptr, const int *col, const double *val, const int *known,
                   int n_known);

/* Same sparsity / constraints / prolongations as the last smg_precompute on this handle, new VALUES already resident in
 * HBM (d_val: device pointer, the caller's CSR order): the whole re-precompute runs on the GPU (fixed-recipe Galerkin
 * products, SELL refresh, coarse inverse).  smg_precompute() takes the same path automatically when it is handed a
 * matrix with an unchanged pattern. */
int smg_precompute_values_device(smg_hierarchy *h, const double *d_val);

/* ---- operator assembly on the device for a fixed connectivity -------------------------
 * What the callers do with libigl around the solve every time step (05_example_mean_curvature_flow/main.cpp:66-69:
 * massmatrix(U), LHS = M - delta L, RHS = M U; 03_mg_solver/main.cpp:44-61) -- here as three kernels on new vertex
 * positions that never leave HBM.  Values are bit-identical to smg_mesh_cotmatrix / smg_mesh_massmatrix. */
typedef struct smg_assembler smg_assembler;
int smg_assembler_create(const int *F, int nF, int nV, smg_assembler **out);
void smg_assembler_destroy(smg_assembler *a);
/* CSR pattern of the assembled matrix (== the pattern of smg_mesh_cotmatrix); query nnz with NULL arrays first */
int smg_assembler_pattern(const smg_assembler *a, int *nnz, int *rowptr, int *col);
/* d_V: nV x 3 row-major (device).  d_val[nnz] = mass_coef * M + lap_coef * L with L the (negative semi-definite) cotangent
 * matrix and M the lumped mass matrix (voronoi != 0: mixed Voronoi areas, else barycentric); d_mass[nV] (optional) = diag M;
 * d_Lval[nnz] (optional) = L alone.  hip_stream: stream to enqueue on (NULL = default stream). */
int smg_assemble(smg_assembler *a, const double *d_V, int voronoi, double mass_coef, double lap_coef, double *d_val,
                 double *d_mass, double *d_Lval, void *hip_stream);

/* ---- min_quad_with_fixed_mg_solve (src/min_quad_with_fixed_mg.h:38-69 and :79-113) ------------------------------ */
/* RHS, z0, z: n x k column-major (n = full size incl. known rows); known_val: n_known x k (ignored without
 * constraints).  r_his must hold opts->max_iter doubles (any max_iter >= 0, as in the reference, .cpp:77); *n_his <= max_iter entries are written, one per loop
 * entry incl. the one that triggers the break (.cpp:108-116).  *converged = !(last measured residual > tol)
 * (.cpp:131-134).  memspace: SMG_HOST or SMG_DEVICE for RHS/known_val/z0/z (r_his is always host). */
int smg_solve(smg_hierarchy *h, const double *RHS, int ld_rhs, const double *known_val, int ld_kv, const double *z0,
              int ld_z0, int k, int memspace, const smg_solve_opts *opts, double *z, int ld_z, double *r_his,
              int *n_his, int *converged);

/* The same system solved by conjugate gradients with one V-cycle as the preconditioner (an addition: the reference has no Krylov solver).
 * Flexible (Polak-Ribiere) PCG, one independent recurrence per column -- the V-cycle is not symmetric (pre- and post-smoothing sweep in the
 * same order; the fp32 cycle of precision = 1 rounds), and the flexible beta tolerates that:
 *     x = z0_u;  r = RHS_u - A x
 *     loop entry i:  record |r|_F (all columns); if |r|_F < tol: break
 *                    z = V(r, 0);  beta = -alpha_prev (z.q_prev) / rz_prev  (0 in the first iteration and after a restart);  p = z + beta p
 *                    q = A p;  alpha = (z.r) / (p.q);  x += alpha p;  r -= alpha q
 * Every division by an exact zero gives 0 (a zero column stays exactly zero).  V is what smg_solve's cycle is with the same opts (pre, post,
 * smoother, precision); with precision = 1 the cycle runs in fp32 and everything else in fp64.
 * Arguments, memspace, known_val, opts (tol, max_iter, check_every, use_graph, verbosity, ...), r_his, n_his and converged mean what they mean
 * for smg_solve, and the history has its shape: one entry per loop entry, including the one that triggers the break; max_iter = 0 returns
 * z = z0 and *n_his = 0.
 *   r_his[0] is the true residual of z0, measured as smg_solve measures it (the same value as smg_solve's r_his[0]).  Later entries are the
 *   norms of the recurrence's r.  When one of them passes the break test, the true residual of x is computed and replaces that entry; if it
 *   is still >= tol and entries remain, the iteration restarts from x with r = the true residual (beta = 0).  So an entry that ended the loop
 *   is always a true residual, and *converged = !(last entry > tol) as for smg_solve.  A non-finite norm ends the loop with SMG_ERR_NONFINITE.
 * Union handles (smg_union_members > 0) are refused with SMG_ERR_INVALID, as is a call during a split-phase solve.  The Krylov vectors (five
 * n x k blocks) are allocated by the first call; smg_debug_device_bytes lists them as "krylov". */
int smg_solve_pcg(smg_hierarchy *h, const double *RHS, int ld_rhs, const double *known_val, int ld_kv, const double *z0,
                  int ld_z0, int k, int memspace, const smg_solve_opts *opts, double *z, int ld_z, double *r_his,
                  int *n_his, int *converged);

/* The nev smallest eigenpairs of A_uu x = lambda M_uu x (an addition: the reference has no eigensolver).  A_uu is the unknown system the
 * handle was precomputed with; it must be symmetric positive definite (known rows act as Dirichlet rows).  M = diag(mass_diag) restricted to
 * the unknown rows: mass_diag holds n entries in the caller's numbering (block hierarchies: one per DOF), and every unknown row needs a finite
 * mass > 0, else SMG_ERR_INVALID before anything of the handle changes.  Method: LOBPCG (Knyazev 2001) with the basis selection of
 * Hetmaniuk and Lehoucq (2006), preconditioned by W = V(R, 0) -- one V-cycle with opts' pre / post / smoother; precision = 1 runs the cycle
 * in fp32 and everything else in fp64.
 *   block: m iterated columns, nev <= m <= 64 (the extra columns are guard vectors and are never tested).  0 selects the smallest of
 *          8, 16, 32, 64 that is >= nev + max(2, nev / 4) (at most 64, at most the number of unknowns, at least nev).
 *   X0:    n x m start (column-major, caller numbering, leading dimension ld_x0; all m = block columns are read -- with block = 0 that is
 *          the default block, not nev), or NULL: start column c, row r = a counter-based hash of
 *          (seed, r, c) (splitmix64 finaliser, uniform in [-1, 1)), the same for every memspace.
 *   evals: the nev smallest Ritz values, ascending (host).  X: n x nev, leading dimension ld_x, caller numbering, M-orthonormal
 *          (X^T M X = I), known rows exactly 0.  Within a cluster of equal eigenvalues any M-orthonormal basis of the eigenspace is correct.
 *   res_his (host, NULL allowed): res_his[i * nev + j] = |A x_j - lambda_j M x_j|_{M^-1} / |lambda_j| (x_j^T M x_j = 1) at iteration i; row 0
 *          is the Rayleigh-Ritz of the start.  It must hold (opts->max_iter + 1) * nev doubles; *n_iter = rows written.  Pair j is converged
 *          when its residual <= opts->tol; the loop ends when pairs 0 .. nev-1 all are, or after opts->max_iter iterations.
 *          *n_converged = the number of leading converged pairs.  Not converged is not an error (SMG_OK, as smg_solve).
 *   memspace: where mass_diag, X0 and X live (SMG_HOST / SMG_DEVICE).
 * A non-finite residual or Gram entry returns SMG_ERR_NONFINITE.  SMG_ERR_INVALID: a union handle, a call during a split-phase solve,
 * nev < 1, block < nev or > 64, fewer unknowns than the block.  Every run with the same inputs returns the same bits (memspace, graphs on or
 * off: the loop runs eagerly, one host synchronisation per iteration).  Nothing smg_solve / smg_solve_pcg compute afterwards changes.  The
 * buffers (about ten n x m blocks) are allocated by the first call; smg_debug_device_bytes lists them as "eigs".
 * Closed meshes (A = -L is singular): precompute a shifted matrix.  The mean-curvature-flow system A = M - delta L gives the Laplace-Beltrami
 * eigenvalues of -L x = lambda_L M x as lambda_L = (mu - 1) / delta from its eigenvalues mu; for -L itself, precompute -L + sigma M and
 * subtract sigma.  Not covered: a sparse (non-diagonal) mass matrix, union handles, a column-sharded form. */
int smg_eigs(smg_hierarchy *h, const double *mass_diag, int nev, int block, const double *X0, int ld_x0, int memspace,
             const smg_solve_opts *opts, unsigned long long seed, double *evals, double *X, int ld_x, double *res_his, int *n_iter,
             int *n_converged);

/* ---- geodesic distance by the heat method (Crane, Weischedel, Wardetzky 2013; libigl's heat_geodesics_precompute / _solve) ----------
 * An addition: the reference has no distance query.  One query, per column c of sources S_c:
 *     (M - t L) u = 1_{S_c}                       heat step, Neumann on mesh boundaries
 *     X_f = -grad u / |grad u| per face            (X_f = 0 where grad u == 0)
 *     -L phi = -div X                              Poisson step, vertex 0 pinned at 0
 *     D = phi - mean(phi over S_c)                 so a single source has D = 0 there
 * with L the cotangent matrix (negative semi-definite) and M the lumped mass matrix (voronoi != 0: mixed Voronoi, else barycentric), both
 * assembled on the device (smg_assemble).  Both systems are solved by the V-cycle of the hierarchy the object was created from.
 *
 * smg_geodesics_create: h gives the prolongations (any scalar hierarchy on this mesh: smg_mg_precompute, _subdiv, a file, ...).  They are
 *   copied in memory into two internal handles -- the heat handle (M - tL, no pins) and the Poisson handle (-L, vertex 0 known) -- which are
 *   precomputed here; h is not modified and may be destroyed afterwards.  V: nV x 3 row-major, F: nF x 3.
 *   t > 0 is used as given; t == 0 selects the default t = (d / 12)^2 with d the diagonal of the bounding box of V (DESIGN.md section 18:
 *   libigl's t = h^2 leaves u below the rounding of an iterative solve on the far side of the mesh).  SMG_ERR_INVALID, before any device
 *   work: a null argument, t < 0 or not finite, a union handle, a block (3-DOF) hierarchy, nV != the rows of level 0, a face index out of
 *   range, a face with zero double area, a mesh of more than one connected component.  SMG_ERR_NO_DEVICE without a GPU.
 * smg_geodesics_time: the t in use.
 * smg_geodesics_set_solver: heat_pcg / poisson_pcg = 1 solve that stage with smg_solve_pcg (the default for both: fewer cycles at the tight
 *   tolerances below), 0 with smg_solve's stationary loop; < 0 keeps the current choice.
 * smg_geodesics_device_bytes: the device memory held by the object -- both internal handles (as smg_debug_device_bytes counts them) and
 *   the object's own buffers (gradient basis, corner lists, three n x k blocks, sized by the largest k queried so far).
 * smg_geodesics_solve: k >= 1 source sets, set c = src[src_ptr[c] .. src_ptr[c + 1]) (host arrays; a set must not be empty, indices in
 *   [0, nV), a repeated index counts once in the heat step and once per occurrence in the mean).  D: nV x k column-major, leading dimension
 *   ld_d >= nV, in memspace (SMG_HOST / SMG_DEVICE); everything between the source lists and D stays on the device, on one stream.
 *   heat_opts / poisson_opts: the options of the two solves (tol is absolute, as for smg_solve); NULL selects smg_solve_opts_default with
 *   max_iter = 100 and tol = 1e-11 sqrt(number of source entries) for the heat step (the norm of its right-hand side), 1e-11 sqrt(k A) for
 *   the Poisson step (A = the mesh's area; its right-hand side has that scale).  cycles (NULL ok): the loop entries of the two solves.
 *   A stage that ends unconverged is not an error (as for smg_solve: cycles[i] == max_iter tells); a failing solve's error code (e.g.
 *   SMG_ERR_NONFINITE) is returned unchanged.  Every call with the same inputs returns the same bits (graphs on or off). */
typedef struct smg_geodesics smg_geodesics;
int smg_geodesics_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, double t, int voronoi, smg_geodesics **out);
void smg_geodesics_destroy(smg_geodesics *g);
double smg_geodesics_time(const smg_geodesics *g);
int smg_geodesics_set_solver(smg_geodesics *g, int heat_pcg, int poisson_pcg);
long long smg_geodesics_device_bytes(const smg_geodesics *g);
int smg_geodesics_solve(smg_geodesics *g, int k, const int *src_ptr, const int *src, int memspace, const smg_solve_opts *heat_opts,
                        const smg_solve_opts *poisson_opts, double *D, int ld_d, int *cycles);

/* ---- as-rigid-as-possible deformation (Sorkine and Alexa 2007, spokes energy; libigl's arap_precompute / arap_solve) --------------------
 * An addition: the reference has no deformation.  Rest positions p, deformed positions p', w_ij = L_ij the off-diagonal entries of the
 * cotangent matrix of the REST pose (as smg_assemble produces them), e_ij = p_i - p_j, e'_ij = p'_i - p'_j, N(i) = the off-diagonal
 * entries of row i of L in stored order:
 *     E(R, p') = sum_i sum_{j in N(i)} w_ij |e'_ij - R_i e_ij|^2
 *     local :  S_i = sum_j w_ij e_ij e'_ij^T,  R_i = the rotation (det = +1) that maximises tr(R_i S_i)
 *              = V D U^T for S_i = U Sigma V^T, D = diag(1, 1, det(V U^T)), the flip on the smallest singular value
 *     global:  (-L) p' = b,  b_i = sum_j (w_ij / 2) (R_i + R_j) e_ij,  the rows of the handle vertices known = the handle positions
 * Iteration t: rotations R_t from the iterate U_t, E_t = E(R_t, U_t), the right-hand side, one 3-column solve warm-started at U_t -> U_{t+1}.
 * After the last iteration one more local step gives the last energy (and leaves the final rotations in the object).  With exact solves
 * E_{t+1} <= E_t.  The matrix never changes while handles move: it is precomputed once, at create.
 *
 * smg_arap_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied in memory into one internal handle, which
 *   is precomputed here with -L and known = handles; h is not modified and may be destroyed afterwards.  V: nV x 3 row-major (the rest
 *   pose), F: nF x 3, handles: n_handles distinct vertices (their order is the row order of handle_pos).  SMG_ERR_INVALID, before any
 *   device work: a null argument, n_handles < 1, a handle out of range or repeated, every vertex a handle, a union handle, a block (3-DOF)
 *   hierarchy, nV != the rows of level 0, a face index out of range, a face with zero double area, a non-finite coordinate, a mesh of more
 *   than one connected component.  SMG_ERR_NO_DEVICE without a GPU.  A rest pose whose -L_uu is not positive definite fails in
 *   smg_precompute, with that call's code.
 * smg_arap_set_solver: pcg = 1 the global step runs smg_solve_pcg (the default: at the default tolerance the warm-started solves of the
 *   1 M-vertex benchmark mesh take 7 - 8 loop entries by PCG against 10 - 11 by the stationary loop, 4.5 against 5.1 ms per iteration;
 *   DESIGN.md section 19), 0 smg_solve's stationary loop; < 0 keeps the choice.
 * smg_arap_device_bytes: the device memory held by the object -- the internal handle (as smg_debug_device_bytes counts it) and the
 *   object's own buffers (the CSR of L, positions, rotations, four n x 3 blocks).
 * smg_arap_solve: handle_pos: n_handles x 3 column-major, leading dimension ld_hp.  U0: nV x 3 column-major, or NULL = the rest pose; its
 *   handle rows are ignored (the handle rows of every iterate are handle_pos).  U: nV x 3 column-major, leading dimension ld_u >= nV (rows
 *   past nV are left alone).  handle_pos, U0 and U live in memspace (SMG_HOST / SMG_DEVICE); energy_his, cycles and n_iter are host.
 *   Runs max_iter iterations (>= 0; 0 returns the start and E_0).  rel_tol > 0 ends the loop before iteration t + 1 when
 *   E_t - E_{t+1} <= rel_tol |E_t|; rel_tol == 0 disables that test.  energy_his (NULL ok) must hold max_iter + 1 doubles, *n_iter + 1 are
 *   written; cycles (NULL ok) must hold max_iter ints: the loop entries of each inner solve; *n_iter (NULL ok): the iterations run.
 *   opts: the options of the inner solves (tol is absolute, as for smg_solve); NULL selects smg_solve_opts_default with max_iter = 50 and
 *   tol = 1e-8 s, s = sqrt(sum_i (sum_j |w_ij| |e_ij|)^2), computed once at create: |R e| = |e|, so s bounds |b|_F for every set of
 *   rotations and the default does not depend on the deformation.  An inner solve that ends unconverged is not an error
 *   (cycles[t] == opts->max_iter tells); a failing solve's code is returned unchanged; a non-finite energy returns SMG_ERR_NONFINITE.
 *   Everything between handle_pos / U0 and U stays on the object's stream; per iteration the host reads one energy double beside the inner
 *   solve's own history.  Every call with the same inputs returns the same bits (graphs on or off, SMG_HOST or SMG_DEVICE).
 * Not covered: the spokes-and-rims and element energies, dynamics, a new handle SET without a new object, union / block / sharded forms;
 * negative cotangent weights are used as they are. */
typedef struct smg_arap smg_arap;
int smg_arap_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const int *handles, int n_handles, smg_arap **out);
void smg_arap_destroy(smg_arap *a);
int smg_arap_set_solver(smg_arap *a, int pcg);
long long smg_arap_device_bytes(const smg_arap *a);
int smg_arap_solve(smg_arap *a, const double *handle_pos, int ld_hp, const double *U0, int ld_u0, int memspace, int max_iter, double rel_tol,
                   const smg_solve_opts *opts, double *U, int ld_u, double *energy_his, int *cycles, int *n_iter);

/* ---- implicit-Euler steps of a pressurised membrane, neo-Hookean by default (the reference's 06_example_balloon_sim: main.cpp:109-134,
 * implicit_euler_mg_balloon.h:35-121, stretching energy only, no constraints) -- an application object on the BLOCK V-cycle -----------------
 * Per face with corners q0, q1, q2 (order of F), e1 = q1 - q0, e2 = q2 - q0:  a = [[e1.e1, e1.e2], [e1.e2, e2.e2]], abar = a of the rest pose,
 *     lnJ = log(det a / det abar) / 2,   W_f = coeff (beta (tr(abar^-1 a) - 2 - 2 lnJ) + alpha lnJ^2),   coeff = thickness sqrt(det abar) / 4,
 *     alpha = young poisson / (1 - poisson^2),  beta = young / (2 (1 + poisson)).
 * G_f (9) and H_f (9 x 9) are its derivatives with respect to (q0, q1, q2) (NeoHookeanMaterial.cpp:12-68); every eigenvalue of H_f below
 * eig_floor is replaced by eig_value (ElasticShell.cpp:86-95), so H = M + dt^2 K is positive definite.  K and g sum the faces' blocks.
 * A step from the state (pos, qdot), qdot0 = qdot, pos0 = pos:
 *     fext_v = -pressure m_v(pos) n_v(pos)      m: lumped Voronoi mass of the CURRENT pose, n: unit vertex normal (area-weighted face normals)
 *     M = mass_scale (Voronoi mass of the REST pose), three equal entries per vertex
 *     newton_iters times:  (G, K) at pos;  H = M + dt^2 K;  b = -(M (qdot - qdot0) + dt G + dt fext)
 *         value-only re-precompute with H;  dx = solve(H, b) from 0
 *         f(t) = sum_v (pos0_v + dt t_v) . fext_v + (t - qdot0)^T M (t - qdot0) / 2 + W(pos0 + dt t)
 *         s = f(qdot) + ls_c b . dx;  a = 1;  while a > ls_min_alpha: if f(qdot + a dx) <= s: qdot += a dx, stop;  else a *= ls_shrink
 *         pos = pos0 + dt qdot
 * The acceptance test is the reference's (b is the NEGATIVE gradient, so it is weaker than Armijo's); when the search gives up qdot is left
 * alone.  When |b|_F is below the solve's tolerance the solve returns dx = 0 after one loop entry and a = 1 is accepted.
 *
 * smg_membrane_create: h must be a block hierarchy on this mesh (level 0 has 3 nV rows, every prolongation Pv (x) I_3: smg_mg_precompute_block,
 *   smg_level_set_prolong, a file); its prolongations are copied into one internal handle, h is not modified.  The pattern is
 *   (adjacency + I) (x) 1_3x3; the first precompute takes H of the rest pose (assembled on the device), every later one is
 *   smg_precompute_values_device.  The state starts as (V, 0).  SMG_ERR_INVALID before any device work: a null argument, a scalar hierarchy, a
 *   union handle, 3 nV != rows of level 0, a face index out of range, a face of zero double area, a non-finite coordinate, more than one
 *   connected component, dt <= 0, |poisson| >= 1, young <= 0, thickness <= 0, mass_scale <= 0, newton_iters < 0, eig_value <= 0.
 * smg_membrane_set_state / get_state: nV x 3 row-major blocks (host or device); set: NULL pos = the rest pose, NULL qdot = 0; get: NULL = skip.
 * smg_membrane_set_solver: 0 (default) smg_solve, the reference's loop; 1 smg_solve_pcg.
 * smg_membrane_set_material: 0 (default) the neo-Hookean energy above, 1 StVK (StVKMaterial.cpp:11-60), 2 tension-field StVK
 *   (TensionFieldStVKMaterial.cpp:11-171): the materials of the reference's runSimulation (main.cpp:92-101).  With M = abar^-1 (a - abar),
 *   c = thickness sqrt(det abar) / 8:  StVK is W_f = c (alpha / 2 tr(M)^2 + beta tr(M^2)); it is finite for inverted faces.  Tension field:
 *   l1 >= l2 the eigenvalues of M, k1 = thickness alpha / 8, k2 = thickness beta / 4;  l1 >= 0 and l2 >= -k1 / (k1 + k2) l1: StVK (pure
 *   tension, the rest pose included);  else l1 < 0: W_f = 0, G_f = 0, H_f = 0 (slack; the fixed block is eig_value I_9);  else
 *   W_f = (k1 + k2 - k1^2 / (k1 + k2)) sqrt(det abar) / 2 l1^2 (wrinkled: no resistance to compression across the wrinkles).  Everything
 *   else of the step is the same.  The int is latched: legal between any two steps, the state is kept, nothing is rebuilt (every Newton
 *   iteration re-precomputes the values anyway).  Any other value, or a null object: SMG_ERR_INVALID.  smg_membrane_material returns the
 *   current one (0 for a null object).
 * smg_membrane_step: opts == NULL selects smg_solve_opts_default with tol = 2e-1 (the reference's mg_tolerance; the tolerance is absolute).
 *   Outputs (NULL ok): objective_his[i] = f(qdot) before Newton iteration i plus one final entry (newton_iters + 1 doubles), alpha[i] the
 *   accepted step (0 when the search gave up), cycles[i] the loop entries of solve i, *n_newton the iterations completed.  A non-finite
 *   objective at an accepted state (a face with det a <= 0 has W = +inf) returns SMG_ERR_NONFINITE; a trial state with one simply fails the
 *   acceptance test.  A failing solve's code is returned unchanged.  The same inputs give the same bits.
 * smg_membrane_lists: the block pattern and the contribution lists the matrix kernel sums in: bptr[nV + 1] / bcol[n_blocks] the block CSR
 *   (columns ascending), c_ptr[n_blocks + 1] / c_src[9 nF] per block the sub-blocks 9 f + 3 a + b (corners a, b of face f), faces ascending.
 *   Query the sizes with NULL arrays first.  Scalar row 3 i + l of H holds, for the blocks q of block row i in order, the columns
 *   3 bcol[q] + m, m = 0 .. 2.
 * smg_membrane_faces_host: the per-face maths of the device kernel compiled for the host (no device needed): W[nF], G (9 planes, entry e of
 *   face f at G[e nF + f], may be NULL with H), H (the 45 entries of the upper triangle row by row, same planes, may be NULL), fixed when fix != 0.
 * smg_membrane_faces_host_material: the same for a material (0: the bits of smg_membrane_faces_host; another value: SMG_ERR_INVALID). */
typedef struct {
    double young, poisson, thickness, mass_scale, dt, pressure;
    int newton_iters;
    double ls_c, ls_shrink, ls_min_alpha, eig_floor, eig_value;
} smg_membrane_params;
void smg_membrane_params_default(smg_membrane_params *p);   /* 6e6, .5, .1, 1000, 1e-3, 1e6, 10, 1e-8, .5, 1e-8, 1e-6, 1e-3 */
typedef struct smg_membrane smg_membrane;
int smg_membrane_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const smg_membrane_params *p, smg_membrane **out);
void smg_membrane_destroy(smg_membrane *m);
long long smg_membrane_device_bytes(const smg_membrane *m);
int smg_membrane_set_state(smg_membrane *m, const double *pos, const double *qdot, int memspace);
int smg_membrane_get_state(smg_membrane *m, double *pos, double *qdot, int memspace);
int smg_membrane_set_solver(smg_membrane *m, int pcg);
int smg_membrane_set_material(smg_membrane *m, int material);
int smg_membrane_material(const smg_membrane *m);
int smg_membrane_step(smg_membrane *m, const smg_solve_opts *opts, double *objective_his, double *alpha, int *cycles, int *n_newton);
int smg_membrane_lists(const int *F, int nF, int nV, int *n_blocks, int *n_contrib, int *bptr, int *bcol, int *c_ptr, int *c_src);
int smg_membrane_faces_host(const double *V0, const double *P, int nV, const int *F, int nF, const smg_membrane_params *p, int fix, double *W,
                            double *G, double *H);
int smg_membrane_faces_host_material(const double *V0, const double *P, int nV, const int *F, int nF, const smg_membrane_params *p, int material,
                                     int fix, double *W, double *G, double *H);

/* ---- harmonic and as-rigid-as-possible flattening of a disk mesh (Tutte / cotangent-weight harmonic map to a circle; the local / global
 * iteration of Liu, Zhang, Xu, Gotsman and Gortler 2008) -- an application object on a SCALAR hierarchy --------------------------------------
 * An addition: the reference has no parameterization.  u is the nV x 2 map.
 * Rest triangle: face f has corners p0, p1, p2 in the order of F, e1 = p1 - p0, e2 = p2 - p0; its isometric rest triangle in the plane is
 *     x0 = (0, 0),  x1 = (|e1|, 0),  x2 = (e1 . e2 / |e1|, |e1 x e2| / |e1|).
 * Weights: c_i, i = 0, 1, 2, is the cotangent of the angle at corner i + 2 (mod 3), the corner opposite edge (i, i + 1), computed from the rest
 *     triangle.  With these weights -L of smg_assemble is (1/2) sum_f c_i on that edge: the matrix the other objects use.
 * Energy:      E(R, u) = (1/2) sum_f sum_i c_i |(u_i - u_{i+1}) - R_f (x_i - x_{i+1})|^2
 * Local step:  S_f = sum_i c_i (u_i - u_{i+1}) (x_i - x_{i+1})^T,  a = S00 + S11,  b = S10 - S01,  h = sqrt(a^2 + b^2),
 *              R_f = [[a, -b], [b, a]] / h, the identity when h == 0.
 * Global step: (-L) u = rhs,  rhs_v = sum over the faces at v, v being corner i, of (1/2) R_f (c_i (x_i - x_{i+1}) + c_{i-1} (x_i - x_{i-1}));
 *              one vertex, the first of the boundary loop, is known with the value it has in the iterate.
 * Iteration t: rotations from U_t, E_t, the right-hand side, then one 2-column solve warm-started at U_t.  After the last iteration one more
 *     local step gives the last energy.  Negative cotangents are used as they are; -L is the Dirichlet form and stays semi-definite.  With
 *     exact solves E_{t+1} <= E_t.
 * Harmonic start: the longest boundary loop, as smg_mesh_boundary_loop returns it, goes to the circle of the mesh's area (radius
 *     sqrt(area / pi)); the points are placed by cumulative 3D edge length, starting at angle 0 (libigl's map_vertices_to_circle, scaled);
 *     (-L)_uu u = -(-L)_ub u_b, 2 columns, from zero.
 * Distortion of a map, per face: J = [u1 - u0, u2 - u0] [x1, x2]^-1, det J, and the singular values in closed form,
 *     Q = (1/2) sqrt((J00 + J11)^2 + (J10 - J01)^2),  T = (1/2) sqrt((J00 - J11)^2 + (J10 + J01)^2),  sigma1 = Q + T,  sigma2 = |Q - T|;
 *     a face is flipped when det J <= 0.
 * UV blocks are nV x 2 column-major with a leading dimension >= nV; memspace is SMG_HOST or SMG_DEVICE.
 *
 * smg_param_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied in memory into two internal handles, both
 *   precomputed here with -L: one with the boundary loop known (the harmonic map), one with the loop's first vertex known (the global step).
 *   h is not modified and may be destroyed afterwards.  V: nV x 3 row-major, F: nF x 3.  The rest triangles, the weights, the vertex ->
 *   (face, corner) lists (faces ascending) and the scales of the default tolerances are computed here.  SMG_ERR_INVALID, before any device
 *   work: a null argument, a union handle, a block (3-DOF) hierarchy, nV != the rows of level 0, a face index out of range, a face with zero
 *   double area, a non-finite coordinate, a mesh of more than one connected component; then the object's own checks, each with its own
 *   message: an edge shared by more than two faces (or by two faces in the same direction), a closed mesh, more or fewer than one boundary
 *   loop (an annulus), an Euler characteristic other than 1 (handles), every vertex on the boundary.  SMG_ERR_NO_DEVICE without a GPU.
 * smg_param_set_solver: pcg = 1 the solves run smg_solve_pcg (the default), 0 smg_solve's stationary loop; < 0 keeps
 *   the choice.
 * smg_param_device_bytes: the device memory held by the object -- both internal handles (as smg_debug_device_bytes counts them) and the
 *   object's own buffers (faces, corner lists, 18 per-face planes, three nV x 2 blocks).
 * smg_param_boundary: *n_loop (NULL ok) = the length of the boundary loop, loop (NULL ok; n_loop ints) = its vertices in order.
 * smg_param_harmonic: the harmonic start into UV.  opts: the options of the solve (tol is absolute, as for smg_solve); NULL selects
 *   smg_solve_opts_default with max_iter = 50 and tol = 1e-8 s, s the Frobenius norm of the reduced right-hand side -(-L)_ub u_b, computed
 *   once at create.  *cycles (NULL ok): the loop entries of the solve.  The boundary rows of UV are the circle positions themselves.
 * smg_param_arap: UV0: the start, or NULL = the harmonic map, computed inside with the same opts.  Runs max_iter iterations (>= 0; 0
 *   returns the start and E_0).  rel_tol > 0 ends the loop before iteration t + 1 when E_t - E_{t+1} <= rel_tol |E_t|; rel_tol == 0 disables
 *   that test.  energy_his (NULL ok) must hold max_iter + 1 doubles, *n_iter + 1 are written; cycles (NULL ok) must hold max_iter ints: the
 *   loop entries of each inner solve; *n_iter (NULL ok): the iterations run.  opts == NULL selects smg_solve_opts_default with max_iter = 50
 *   and tol = 1e-8 s, s = sqrt(sum_v (sum over the faces at v of (1/2) (|c_i| |x_i - x_{i+1}| + |c_{i-1}| |x_i - x_{i-1}|))^2), computed once
 *   at create: it bounds |rhs|_F for every set of rotations.  An inner solve that ends unconverged is not an error (cycles[t] ==
 *   opts->max_iter tells); a failing solve's code is returned unchanged; a non-finite energy returns SMG_ERR_NONFINITE.  Everything between
 *   UV0 and UV stays on the object's stream; per iteration the host reads one energy double beside the inner solve's own history.  Every
 *   call with the same inputs returns the same bits (graphs on or off, SMG_HOST or SMG_DEVICE).
 * smg_param_distortion: sigma (NULL ok; in memspace) holds 2 nF doubles in planes, sigma1 then sigma2.  stats is a host array of 6 doubles:
 *   the number of flipped faces; max sigma1 / sigma2 over the unflipped faces; the rest-area-weighted mean of sigma1 / sigma2 (all faces);
 *   the same mean of sigma1 sigma2; the rest-area-weighted mean over the unflipped faces of the symmetric Dirichlet density
 *   sigma1^2 + sigma2^2 + sigma1^-2 + sigma2^-2 (NaN when every face is flipped); the total rest area.  The sums are fixed-order reductions,
 *   the maximum goes through a tree of the same shape.
 * Not covered: free-boundary conformal maps (LSCM / ASAP), SLIM and other flip-free energies; meshes with several boundary loops or
 * handles, seams and cuts; boundary shapes other than the circle; union / block / sharded forms. */
typedef struct smg_param smg_param;
int smg_param_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, smg_param **out);
void smg_param_destroy(smg_param *p);
int smg_param_set_solver(smg_param *p, int pcg);
long long smg_param_device_bytes(const smg_param *p);
int smg_param_boundary(const smg_param *p, int *n_loop, int *loop);
int smg_param_harmonic(smg_param *p, int memspace, const smg_solve_opts *opts, double *UV, int ld_uv, int *cycles);
int smg_param_arap(smg_param *p, const double *UV0, int ld_uv0, int memspace, int max_iter, double rel_tol, const smg_solve_opts *opts,
                   double *UV, int ld_uv, double *energy_his, int *cycles, int *n_iter);
int smg_param_distortion(smg_param *p, const double *UV, int ld_uv, int memspace, double *sigma, double *stats);

/* ---- projective-dynamics membrane steps on the scalar V-cycle (csrc/smg_pd.cpp; Bouaziz, Martin, Liu, Kavan, Pauly
 * 2014, triangle-strain constraints).  The global matrix (density / dt^2) M0 - stiffness L of the rest pose (Voronoi mass) is the same for x, y
 * and z and constant for the life of the object: one precompute at create, none afterwards.  The per-face maths (rest frame, deformation
 * gradient, the closed-form 3 x 2 singular-value projection onto the band [sigma_min, sigma_max], its two guards) is stated in
 * csrc/smg_pd_inl.hpp.  One step of size h = dt from (x, v), n_pins >= 0 pinned vertices:
 *   f_v = pressure m_v(x) n_v(x) + density m0_v g (m_v the mixed Voronoi mass of the start pose, n_v the unit vector along the sum of e1 x e2
 *   over the vertex's corners, m0 the mass of the rest pose); s_v = x_v + h v_v + h^2 f_v / (density m0_v), a pinned row takes its pin position;
 *   q_0 = s; iteration t: T_f = the projection of F_f(q_t), E_t = sum_v (density m0_v / (2 h^2)) |q_v - s_v|^2 + sum_f (stiffness A_f / 2)
 *   |F_f(q_t) - T_f|_F^2, then ((density / h^2) M0 - stiffness L) q_{t+1} = b, b_v = (density m0_v / h^2) s_v + the sum over v's corners (f, i),
 *   list order, of stiffness A_f (T_f g_{f,i}), pinned rows known: one 3-column solve warm-started at q_t.  Then v = (q - x) / h, x = q.
 *   With exact solves E_{t+1} <= E_t.  sigma_min = sigma_max = 1 is the ARAP membrane; a wider band limits strain.
 * smg_pd_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied into one internal handle, h is not modified.
 *   dt, density and stiffness are in the matrix and fixed at create.  pins (n_pins >= 0 distinct vertices; NULL when 0) are held at rest until
 *   a step moves them.  The state starts as (V, 0).  SMG_ERR_INVALID, before any device work, for: a union or block hierarchy, nV that is not the
 *   hierarchy's level-0 rows, a face index out of range, a face of zero area, a non-finite coordinate, more than one connected component;
 *   then dt, density or stiffness non-finite or <= 0; strain limits non-finite or not 0 <= sigma_min <= sigma_max; non-finite pressure or
 *   gravity; a pin out of range or repeated; every vertex pinned.  SMG_ERR_NO_DEVICE comes after all of them.
 * smg_pd_set_solver: pcg = 1 the solves run smg_solve_pcg (the default), 0 smg_solve's stationary loop; < 0 keeps.
 * smg_pd_set_state / smg_pd_get_state: pos, vel are nV x 3 xyz rows in memspace; NULL keeps (set) or is skipped (get).
 * smg_pd_set_forces (gravity: 3 doubles on the host, NULL keeps) and smg_pd_set_strain_limits: legal between any two steps; nothing is rebuilt.
 * smg_pd_step: pin_pos (n_pins x 3 xyz rows in memspace; NULL keeps the pins where they are) are the pin positions at the END of the step.
 *   The loop and its stopping rule are those of smg_arap_solve: max_iter iterations (>= 0), rel_tol > 0 ends earlier when
 *   E_{t-1} - E_t <= rel_tol |E_{t-1}|; energy_his (max_iter + 1 doubles), cycles (max_iter ints: the loop entries of each inner solve) and
 *   n_iter may be NULL.  opts: the options of the inner solves (tol is absolute); NULL selects smg_solve_opts_default with max_iter = 50 and
 *   tol = 1e-8 |b_0|_F of this step (all rows).  An unconverged inner solve is not an error; a failing solve's code is returned unchanged.  A
 *   non-finite energy returns SMG_ERR_NONFINITE and leaves the state and the pins as they were before the call.  The same inputs give the
 *   same bits with graphs on or off and with SMG_HOST or SMG_DEVICE.
 * smg_pd_strain: of the current state.  sigma (NULL ok; in memspace) holds 2 nF doubles in planes, sigma1 then sigma2.  stats is a host array
 *   of 4 doubles: max sigma1, min sigma2, the number of faces outside the band (sigma1 > sigma_max or sigma2 < sigma_min), the
 *   rest-area-weighted mean of |F - T|_F^2.  The sums are fixed-order reductions, max and min go through a tree of the same shape.
 * smg_pd_project_host: the host twin of the face maths (no GPU): of the pose P (nV x 3 xyz rows) against the rest pose V0, the planes Fg (6:
 *   f1x, f1y, f1z, f2x, f2y, f2z), sigma (2) and T (6, as Fg), each NULL ok; *guard_hits (NULL ok) = the faces on which a guard fired.
 * Not covered: bending, collisions, per-face stiffness or thickness, volume constraints, several components, union / block / sharded forms,
 * Chebyshev or other acceleration of the outer iteration. */
typedef struct smg_pd smg_pd;
typedef struct { double dt, density, stiffness, sigma_min, sigma_max, pressure, gravity[3]; } smg_pd_params;
void smg_pd_params_default(smg_pd_params *p);              /* 1e-2, 1, 1, 1, 1, 0, {0,0,0} */
int smg_pd_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const int *pins, int n_pins, const smg_pd_params *p,
                  smg_pd **out);
void smg_pd_destroy(smg_pd *d);
long long smg_pd_device_bytes(const smg_pd *d);
int smg_pd_set_solver(smg_pd *d, int pcg);
int smg_pd_set_state(smg_pd *d, const double *pos, const double *vel, int memspace);
int smg_pd_get_state(smg_pd *d, double *pos, double *vel, int memspace);
int smg_pd_set_forces(smg_pd *d, double pressure, const double *gravity);
int smg_pd_set_strain_limits(smg_pd *d, double sigma_min, double sigma_max);
int smg_pd_step(smg_pd *d, const double *pin_pos, int memspace, int max_iter, double rel_tol, const smg_solve_opts *opts, double *energy_his,
                int *cycles, int *n_iter);
int smg_pd_strain(smg_pd *d, int memspace, double *sigma, double *stats);
int smg_pd_project_host(const double *V0, const double *P, int nV, const int *F, int nF, double sigma_min, double sigma_max, double *Fg,
                        double *sigma, double *T, int *guard_hits);

/* ---- feature-preserving denoising on the scalar V-cycle (csrc/smg_denoise.cpp): the bilateral normal filter of Zheng,
 * Fu, Au, Tai 2011 (local scheme), then vertex positions that follow the filtered normals.  The global matrix fidelity M - L of the input mesh
 * (Voronoi mass) is the same for x, y and z and constant for the life of the object: one precompute at create, none afterwards.  All of the
 * following are taken from the input mesh (V, F) and stay fixed: the unit face normals n_f, the areas A_f, the centroids c_f, w_{f,k} = half the
 * cotangent at corner k (the weight of the edge opposite corner k, the convention of smg_mesh_cotmatrix), the mass M, and N(f) = the faces that
 * share at least one vertex with f, without f, ascending (smg_mesh_face_neighbours).  The per-face maths is stated in csrc/smg_denoise_inl.hpp.
 *   Filter: from m^0 (the argument; NULL: n), normal_iters times: s_f = sum over g in N(f), list order, of A_g exp(-|c_f - c_g|^2 / (2 sigma_s^2))
 *   exp(-|m_f - m_g|^2 / (2 sigma_r^2)) m_g (one exponential of the summed arguments), m_f <- s_f / |s_f|; |s_f| zero or not finite: m_f stays.
 *   Every face reads the old normals.
 *   Update: the alternating minimisation of E(X, t) = (1/2) sum_f sum_k w_{f,k} |(x_i - x_j) - t_{f,k}|^2 + (fidelity / 2) sum_v M_v |x_v - V_v|^2
 *   with every t_{f,k} orthogonal to m_f, (i, j) the two corners after k in cyclic order.  Iteration t: h_{f,k} = (x_i - x_j) . m_f,
 *   t_{f,k} = (x_i - x_j) - h_{f,k} m_f, E_t = sum_f (1/2) sum_k w_{f,k} h_{f,k}^2 + the fidelity term; then (fidelity M - L) x_{t+1} =
 *   fidelity M V + b, b_v = the sum over v's corners, list order, of +w_{f,k} t_{f,k} where v is i and -w_{f,k} t_{f,k} where v is j: one 3-column
 *   solve warm-started at x_t.  With exact solves E_{t+1} <= E_t.
 * smg_denoise_params: sigma_s <= 0 selects the rule sigma_s = the mean of |c_f - c_g| over all ordered pairs (f, g in N(f)), a fixed-order sum
 *   computed once at create (a mesh of one face: 1); sigma_r is a distance between unit normals; fidelity has units 1 / length^2, so a value
 *   tuned on one mesh carries over to another only at the same scale: bring the mesh to unit area first (smg_mesh_normalize_unit_area), which
 *   is the scale the default 1 is meant for.  fidelity is in the matrix and fixed at create.
 * smg_denoise_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied into one internal handle, h is not
 *   modified.  SMG_ERR_INVALID, before any device work, for: a union or block hierarchy, nV that is not the hierarchy's level-0 rows, a face
 *   index out of range, a face of zero area, a non-finite coordinate, more than one connected component; then sigma_r or fidelity non-finite
 *   or <= 0, a non-finite sigma_s, normal_iters < 0.  SMG_ERR_NO_DEVICE comes after all of them.  Sharded solves are not offered.
 * smg_denoise_set_solver: pcg = 1 the solves run smg_solve_pcg (the default), 0 smg_solve's stationary loop; < 0 keeps.
 * smg_denoise_sigma_s: the value in use.  smg_denoise_set_filter: legal between any two calls, nothing is rebuilt; sigma_s <= 0, sigma_r <= 0
 *   or normal_iters < 0 keeps the current value (normal_iters = 0 is legal: the filter returns its input); a non-finite value is refused.
 * smg_denoise_filter: runs the filter from normals_in (nF x 3 xyz rows in memspace; NULL: n) and latches the result as m; normals_out (nF x 3
 *   xyz rows in memspace) may be NULL.  A failing call leaves m as it was.
 * smg_denoise_update: runs the update against the latched m (before any filter: m = n) from X0 (nV x 3 xyz rows in memspace; NULL: V) into X
 *   (nV x 3 xyz rows in memspace).  The loop and its stopping rule are those of smg_arap_solve and smg_pd_step: max_iter iterations (>= 0),
 *   rel_tol > 0 ends earlier when E_{t-1} - E_t <= rel_tol |E_{t-1}|; energy_his (max_iter + 1 doubles), cycles (max_iter ints: the loop
 *   entries of each inner solve) and n_iter may be NULL.  opts: the options of the inner solves (tol is absolute); NULL selects
 *   smg_solve_opts_default with max_iter = 50 and tol = 1e-8 |b_0|_F of this call.  An unconverged inner solve is not an error; a failing
 *   solve's code is returned unchanged.  A non-finite energy returns SMG_ERR_NONFINITE: X is not written, nothing is latched, nothing is
 *   written past energy_his[*n_iter].  The object keeps no positions: the next call starts from its own X0.
 * smg_denoise_run: smg_denoise_filter(NULL, NULL), then smg_denoise_update(NULL) in one call.
 *   The same inputs give the same bits with graphs on or off and with SMG_HOST or SMG_DEVICE.
 * smg_denoise_faces_host: the host twin of the per-face pieces (no GPU), with the operands of the ops SMG_DN_REST .. SMG_DN_PROJECT of
 *   smg_debug_denoise below.
 * Not covered: collapse prevention (the energy does not resist slivers at high noise), anisotropic or guided filters, the edge-neighbour
 * variant of N(f), union / block / sharded forms, moving connectivity. */
typedef struct smg_denoise smg_denoise;
typedef struct { double sigma_s, sigma_r, fidelity; int normal_iters; } smg_denoise_params;
enum { SMG_DN_REST = 0, SMG_DN_SPACING = 1, SMG_DN_FILTER = 2, SMG_DN_PROJECT = 3, SMG_DN_RHS = 4, SMG_DN_ENERGY = 5 };
void smg_denoise_params_default(smg_denoise_params *p);    /* 0, 0.35, 1, 20 */
int smg_denoise_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const smg_denoise_params *p, smg_denoise **out);
void smg_denoise_destroy(smg_denoise *d);
long long smg_denoise_device_bytes(const smg_denoise *d);
int smg_denoise_set_solver(smg_denoise *d, int pcg);
double smg_denoise_sigma_s(const smg_denoise *d);
int smg_denoise_set_filter(smg_denoise *d, double sigma_s, double sigma_r, int normal_iters);
int smg_denoise_filter(smg_denoise *d, const double *normals_in, int memspace, double *normals_out);
int smg_denoise_update(smg_denoise *d, const double *X0, int memspace, int max_iter, double rel_tol, const smg_solve_opts *opts, double *X,
                       double *energy_his, int *cycles, int *n_iter);
int smg_denoise_run(smg_denoise *d, int memspace, int max_iter, double rel_tol, const smg_solve_opts *opts, double *X, double *energy_his,
                    int *cycles, int *n_iter);
int smg_denoise_faces_host(int op, int nV, int nF, const int *F, const double *V0, const double *P, const double *in,
                           const smg_denoise_params *p, double *out);

/* ---- cubic and normal-driven stylization on the scalar V-cycle (csrc/smg_stylize.cpp): Liu and Jacobson 2019 ("Cubic
 * stylization") and its closed-form sibling, Liu and Jacobson 2021 ("Normal-driven spherical shape analogies").  As-rigid-as-possible deformation
 * with a penalty on each vertex's rotated normal.  Rest mesh (V, F); L, w_ij, e_ij, e'_ij, N(i) as for smg_arap above; n_i = the unit
 * area-weighted vertex normal, the normalised sum of (p1 - p0) x (p2 - p0) over the vertex's faces, faces ascending; a_i = the barycentric vertex
 * area, the sum of the double areas over 6 in the same order; lambda_i = a per-vertex weight (uniform lambda unless set); Q = a rotation holding
 * the cube's axes (the identity unless set); t_i = caller-given unit target normals.
 *     cubic:          E(R, U) = sum_i [ (1/2) sum_{j in N(i)} w_ij |e'_ij - R_i e_ij|^2 + lambda_i a_i |Q R_i n_i|_1 ]
 *     normal-driven:  lambda_i a_i |R_i n_i - t_i|^2 in place of the L1 term (Q is not used)
 *     global: (-L) U = b, b_i = sum_j (w_ij / 2) (R_i + R_j) e_ij, the pinned rows known: smg_arap's, the factor 1/2 cancels
 *     local, cubic: S_i = sum_j w_ij e_ij e'_ij^T once, then at most admm_iters iterations from the state (z, u, rho) of the vertex:
 *         M = S + rho n (Q^T (z - u))^T;  R = the closest rotation of M (smg_arap's fit);  y = Q R n;  z_old = z;  z = shrink(y + u, lambda_i a_i / rho);
 *         u += y - z;  r = |z - y|;  s = rho |z - z_old|;  r > mu s: rho *= tau, u /= tau;  else s > mu r: rho /= tau, u *= tau;
 *         stop when r < sqrt(3) abs_tol + rel_tol max(|y|, |z|) and s < sqrt(3) abs_tol + rel_tol rho |u| (the updated rho, u)
 *       z = u = 0 and rho = rho0 at the start of every smg_stylize_run; the state is carried from outer iteration to outer iteration within the
 *       call and nothing is kept between calls: the same inputs give the same bits.
 *     local, normal-driven: R = the closest rotation of S + 2 lambda_i a_i n t_i^T; no state.
 * The paper's edge sets are spokes and rims; this object uses smg_arap's spokes, so that the matrix, the weights and the right-hand side kernel
 * are shared with it.  ADMM does not minimise the local problem exactly, so monotone descent of E is observed, not proved.
 *
 * smg_stylize_params: lambda >= 0; rho0, abs_tol, rel_tol > 0; mu > 1, tau > 1; all finite; admm_iters >= 1.
 * smg_stylize_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied into one internal handle, precomputed here
 *   with -L and known = pins; h is not modified.  pins: n_pins distinct vertices, their order is the row order of pin_pos.  SMG_ERR_INVALID,
 *   before any device work, in this order: a null argument; a union or block hierarchy, nV != the rows of level 0; a face index out of range, a
 *   face of zero area, a non-finite coordinate, more than one connected component; n_pins < 1, a pin out of range or repeated, every vertex
 *   pinned; then the parameters in the order lambda, rho0, abs_tol, rel_tol, mu, tau, admm_iters.  SMG_ERR_NO_DEVICE comes after all of them.
 * smg_stylize_set_solver: as smg_arap_set_solver.  smg_stylize_device_bytes: the internal handle and the object's own buffers.
 * smg_stylize_set_params: legal between calls, nothing is rebuilt; the checks of create.
 * smg_stylize_set_lambda: nV host values lambda_i, each finite and >= 0; NULL: back to the uniform lambda.
 * smg_stylize_set_frame: 9 host doubles, Q row-major; NULL: the identity.  Refused unless |Q^T Q - I| <= 1e-12 entrywise and det Q > 0.
 * smg_stylize_set_targets: nV x 3 host xyz rows of unit vectors select the normal-driven mode; NULL selects the cubic mode.  Refused unless
 *   every row is finite with | |t| - 1 | <= 1e-8.
 * smg_stylize_normals: n (nV x 3 xyz rows) and a (nV) to host arrays; either may be NULL.
 * smg_stylize_run: the start iterate, the local / global loop and the copy out; arguments, memspace handling, stopping rule and
 *   SMG_ERR_NONFINITE exactly as smg_arap_solve (pin_pos for handle_pos); pin_pos may be NULL = the rest positions of the pins.  opts NULL:
 *   smg_solve_opts_default with max_iter = 50 and tol = 1e-8 s, smg_arap's s.
 * smg_stylize_admm_stats: the minimum, mean and maximum of the ADMM iteration counts of the last local step (normal-driven: all 0) and the
 *   number of vertices that used all admm_iters; iters (NULL ok): the nV counts.  Before any run: SMG_ERR_INVALID.
 * smg_stylize_local_host: the host twin of one local step on caller arrays (no GPU, the text the kernels compile), with the operands and the
 *   layout of smg_debug_stylize below; SMG_STY_ENERGY writes the nV terms only.
 * Not covered: the spokes-and-rims energy, per-axis weights, union / block / sharded forms, a new pin SET without a new object. */
typedef struct smg_stylize smg_stylize;
typedef struct { double lambda, rho0, abs_tol, rel_tol, mu, tau; int admm_iters; } smg_stylize_params;
enum { SMG_STY_NORMALS = 0, SMG_STY_ADMM_ONE = 1, SMG_STY_LOCAL = 2, SMG_STY_LOCAL_TARGETS = 3, SMG_STY_ENERGY = 4 };
void smg_stylize_params_default(smg_stylize_params *p);    /* 0.2, 1e-4, 1e-5, 1e-3, 10, 2, 100 */
int smg_stylize_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const int *pins, int n_pins,
                       const smg_stylize_params *p, smg_stylize **out);
void smg_stylize_destroy(smg_stylize *s);
long long smg_stylize_device_bytes(const smg_stylize *s);
int smg_stylize_set_solver(smg_stylize *s, int pcg);
int smg_stylize_set_params(smg_stylize *s, const smg_stylize_params *p);
int smg_stylize_set_lambda(smg_stylize *s, const double *lambda);
int smg_stylize_set_frame(smg_stylize *s, const double *Q);
int smg_stylize_set_targets(smg_stylize *s, const double *targets);
int smg_stylize_normals(smg_stylize *s, double *normals, double *areas);
int smg_stylize_run(smg_stylize *s, const double *pin_pos, int ld_pp, const double *U0, int ld_u0, int memspace, int max_iter, double rel_tol,
                    const smg_solve_opts *opts, double *U, int ld_u, double *energy_his, int *cycles, int *n_iter);
int smg_stylize_admm_stats(smg_stylize *s, int *min_iters, double *mean_iters, int *max_iters, int *at_cap, int *iters);
int smg_stylize_local_host(int op, int nV, int nF, const int *F, const int *rowptr, const int *col, const double *w, const double *V0,
                           const double *P, const double *lambda, const double *Q, const double *targets, const double *state_in,
                           const double *R_in, const smg_stylize_params *p, double *out, int *iters);

/* ---- gradient-domain morphing on the scalar V-cycle (csrc/smg_morph.cpp): Poisson reconstruction from per-face gradients
 * (Yu et al. 2004), pose interpolation through the faces' polar factors (Xu et al. 2005; Alexa et al. 2000), and deformation transfer in the
 * Poisson form of Botsch et al. 2006.  An addition: the reference has none of them.  k sets -- in-between poses, frames -- are 3k right-hand sides
 * of ONE constant matrix with the same pinned rows: a query is one or two face kernels, one vertex kernel and one 3k-column solve.
 *   Rest mesh (V, F): n_f = the rest unit normal of face f, 2A_f its double area, W_fi = (n_f x e_i) / (2A_f) with e_i the edge opposite corner i,
 *     counter-clockwise (e_0 = x_2 - x_1, e_1 = x_0 - x_2, e_2 = x_1 - x_0): the gradient of corner i's hat function, as smg_geodesics forms it.
 *     L = smg_assemble's cotangent matrix of the rest mesh.
 *   Face gradient of a pose X on a rest mesh: T_f = sum_i x_i W_fi^T (i = 0, 1, 2 in order), N_f = the unit normal of the pose face (0 where its
 *     area is 0), J_f = T_f + N_f n_f^T: 3 x 3, row-major.
 *   Polar factors: J_f = R_f S_f, R_f the rotation (det = +1) that maximises tr(R_f^T J_f) = U D V^T for J_f = U Sigma V^T, D = diag(1, 1,
 *     det(U V^T)), the flip on the smallest singular value: smg_arap's one-sided Jacobi and its determinant rule.  S_f = (M + M^T) / 2, M = R_f^T J_f.
 *   Rotation vector: R_f as a unit quaternion (w, v) by Shepperd's branch on the largest of the trace and the three diagonal entries, its sign
 *     chosen so that w >= 0; theta = 2 atan2(|v|, w); omega_f = theta v / |v|, or 0 when |v| = 0.  Stored: 3 + 6 doubles per face (omega_f and
 *     S_f as 00, 01, 02, 11, 12, 22).
 *   Interpolation at time t, any finite t (extrapolation allowed): R_f(t) = Rodrigues' formula for t omega_f, S_f(t) = I + t (S_f - I),
 *     J_f(t) = R_f(t) S_f(t).
 *   Reconstruction: U minimises sum_f A_f |grad u - J_f|_F^2: row i of (-L) U = b with b_i = sum over the corners (f, j) of vertex i, faces
 *     ascending, of A_f J_f W_fj; the pinned rows are known.
 *   Blocks: U, U0 are nV x 3k column-major, pin_pos is n_pins x 3k column-major: column 3c + d is coordinate d of set c.
 *
 * smg_morph_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied into one internal handle, precomputed here,
 *   once, with -L and known = pins; h is not modified.  V: nV x 3 row-major (the rest pose), F: nF x 3, pins: n_pins distinct vertices, their
 *   order is the row order of pin_pos.  SMG_ERR_INVALID, before any device work, in this order: a null argument; a union or block hierarchy,
 *   nV != the rows of level 0; a face index out of range, a face of zero area, a non-finite coordinate, more than one connected component;
 *   n_pins < 1, a pin out of range or repeated, every vertex pinned.  SMG_ERR_NO_DEVICE comes after all of them.
 * smg_morph_set_solver: as smg_arap_set_solver (PCG by default).  smg_morph_device_bytes: the internal handle and the object's own buffers; the
 *   blocks of a query grow with the largest k seen and are kept.
 * The three queries share their last arguments.  pin_pos, U0, U and the query's poses or gradients live in memspace (SMG_HOST / SMG_DEVICE); t,
 *   Fs and cycles are host.  pin_pos NULL and U0 NULL select the defaults named below; the pinned rows of U0 are ignored.  ld_u >= nV (rows past
 *   nV are left alone).  opts: the options of the solve (tol is absolute, as for smg_solve); NULL selects smg_solve_opts_default with max_iter =
 *   100 and tol = 1e-10 |b|_F, |b|_F over all 3k columns (a fixed-order sum, one double read by the host per call).  A sum that is not finite
 *   returns SMG_ERR_NONFINITE before the solve, with nothing written to U.  A solve that ends unconverged is not an error (*cycles ==
 *   opts->max_iter tells; cycles may be NULL); a failing solve's code is returned unchanged.  SMG_ERR_INVALID, before any device work, in this
 *   order: a null argument; k < 1; a bad memspace; a leading dimension that is too small; then what a query adds (a non-finite t).  Every call
 *   with the same inputs returns the same bits (graphs on or off, SMG_HOST or SMG_DEVICE); nothing is kept between calls.
 * smg_morph_reconstruct: J = k sets of nF x 9 row-major gradients (set c at c * 9 nF).  pin_pos NULL: the pins' rest positions in every set;
 *   U0 NULL: the rest pose in every set.
 * smg_morph_interpolate: X = one pose, nV x 3 row-major; t = k times.  pin_pos NULL: (1 - t_c) V[pin] + t_c X[pin]; U0 NULL: the linear blend
 *   (1 - t_c) V + t_c X, the natural warm start.  The polar kernel runs once per call; the right-hand side kernel runs one lane per
 *   (vertex, set) and recomputes J_f(t_c) at every corner: it is never stored.
 * smg_morph_transfer: S0 = the source's rest pose (nVs x 3 row-major), S1 = its k poses (k x nVs x 3), Fs = the source's faces (nF x 3, host):
 *   face f of the source corresponds to face f of the target.  Fs NULL = the object's F, and then nVs must equal nV.  J_f of set c = the face
 *   gradient of pose c on the source's rest mesh (its basis is formed inside the kernel); the solve is on the target's -L with the target's W.
 *   pin_pos and U0 as for reconstruct.  Refused too: Fs NULL with nVs != nV, a source face index out of range.  A source rest face of zero
 *   area makes the sum non-finite.
 * smg_morph_faces_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile), with the operands and the layouts
 *   of smg_debug_morph below.  sin, cos and atan2 are the host's there; everything else is the same correctly rounded arithmetic in one order.
 * Not covered: rotations of more than half a turn (omega_f is the shortest one), a consistent choice of rotation across
 *   neighbouring faces, blends of more than two poses, the search for a source-to-target correspondence, a new pin SET without a new object,
 *   union / block / sharded forms, and degenerate pose faces: where N_f = 0 the result is finite and its accuracy is not stated. */
typedef struct smg_morph smg_morph;
enum { SMG_MORPH_FACE_GRADIENT = 0, SMG_MORPH_FACE_POLAR = 1, SMG_MORPH_RHS_GRADIENT = 2, SMG_MORPH_RHS_INTERP = 3, SMG_MORPH_PINS = 4 };
int smg_morph_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const int *pins, int n_pins, smg_morph **out);
void smg_morph_destroy(smg_morph *m);
int smg_morph_set_solver(smg_morph *m, int pcg);
long long smg_morph_device_bytes(const smg_morph *m);
int smg_morph_reconstruct(smg_morph *m, const double *J, int k, const double *pin_pos, int ld_pp, const double *U0, int ld_u0, int memspace,
                          const smg_solve_opts *opts, double *U, int ld_u, int *cycles);
int smg_morph_interpolate(smg_morph *m, const double *X, const double *t, int k, const double *pin_pos, int ld_pp, const double *U0, int ld_u0,
                          int memspace, const smg_solve_opts *opts, double *U, int ld_u, int *cycles);
int smg_morph_transfer(smg_morph *m, const double *S0, int nVs, const int *Fs, const double *S1, int k, const double *pin_pos, int ld_pp,
                       const double *U0, int ld_u0, int memspace, const smg_solve_opts *opts, double *U, int ld_u, int *cycles);
int smg_morph_faces_host(int op, int nV, int nF, int k, const int *F, const double *V0, const double *X, const double *t, const double *in,
                         const int *pins, int n_pins, double *out);

/* ---- conformalized mean-curvature flow on the scalar V-cycle (csrc/smg_flow.cpp): Kazhdan, Solomon, Ben-Chen 2012, the
 * reference's 05_example_mean_curvature_flow, and the conformal map to the sphere it converges to on a closed genus-0 mesh.  L_0 is the cotangent
 * matrix of the rest mesh, assembled once; step t rebuilds the barycentric mass M_t of the current positions U, solves
 * (M_t - delta L_0) U' = M_t U (three columns, warm-started at U) and, with normalize, applies normalize_unit_area (unit area, x and y means 0,
 * min z 0).  The matrix keeps its pattern: one full smg_precompute at create, smg_precompute_values_device on every step.
 *   sphericity of U: a = the barycentric masses of U, c = sum a_i U_i / sum a_i, r_i = |U_i - c|, rbar = sum a_i r_i / sum a_i,
 *   sqrt(sum a_i (r_i - rbar)^2 / sum a_i) / rbar; 0 on a sphere.  Every sum is a fixed-order reduction.
 * smg_flow_params: delta = the time step (on the unit-area mesh), normalize = 1 normalises the rest mesh at create and the state after every
 *   step, stop_sphericity > 0 ends smg_flow_step once the measured sphericity is at or below it.
 * smg_flow_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied into one internal handle, h is not modified.
 *   SMG_ERR_INVALID, before any device work, for: a union or block hierarchy, nV that is not the hierarchy's level-0 rows, a hierarchy of one
 *   level (smg_precompute_values_device needs two), a face index out of range, a face of zero area, a non-finite coordinate, more than one
 *   connected component; then delta not finite or <= 0, normalize outside
 *   {0, 1}, stop_sphericity not finite or < 0.  SMG_ERR_NO_DEVICE comes after all of them.  V: nV x 3 row-major, as every create takes it.
 * smg_flow_set_params: delta and stop_sphericity of the following steps (the next step's values are formed with the new delta: still value-only);
 *   normalize is fixed at create and a change is refused.  smg_flow_set_solver: as smg_arap_set_solver (PCG by default).
 * smg_flow_step: for t = 0 .. n_steps - 1: the sphericity of the current state into sphericity_his[t]; non-finite: SMG_ERR_NONFINITE; at or below
 *   stop_sphericity (when > 0): SMG_OK; else the step.  After the last step the sphericity once more, into sphericity_his[n_steps].  opts: the
 *   options of the solves (tol is absolute); NULL selects smg_solve_opts_default with tol = 5e-7, what the reference's caller passes.  A solve
 *   that used all of max_iter is not an error (cycles[t] = its loop entries); a failing precompute or solve returns its code unchanged.  Every
 *   end leaves *n_done = t with the state that of t completed steps; nothing is written past sphericity_his[*n_done].  sphericity_his
 *   (n_steps + 1 doubles), cycles (n_steps ints) and n_done may be NULL; n_steps = 0 only measures.  Beside what the solve reads itself the host
 *   reads one double per step.  The same calls give the same bits.
 * smg_flow_positions / smg_flow_set_positions: the state as an nV x 3 column-major block with leading dimension ld_u >= nV in memspace, the
 *   layout of smg_arap_solve's U.  smg_flow_reset: back to the (normalised) rest mesh.
 * smg_flow_sphere: S_i = (U_i - c) / r_i of the current state (nV x 3 column-major, NULL ok); sigma (NULL ok; in memspace) holds 2 nF doubles in
 *   planes, sigma1 then sigma2: the singular values of the 3 x 2 Jacobian that takes the rest face to the sphere face.  stats is a host array of 4
 *   doubles: the rest-area-weighted mean of sigma1 / sigma2 (1 = conformal), its maximum, the number of flipped faces (n_f . centroid_f <= 0 on
 *   the sphere), the sphericity of the state.  SMG_ERR_INVALID for a mesh with a boundary edge, a non-manifold edge or nV - nE + nF != 2
 *   (checked on F at create).
 * smg_flow_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with
 *   the operands and the layouts of smg_debug_flow below.
 * Not covered: the classical flow with L re-assembled from the current positions (its faces degenerate within a few steps and the assembly is
 * refused), Voronoi masses, Moebius centring of the sphere map, pinned vertices, union / block / sharded forms, meshes whose rest faces are
 * already degenerate. */
typedef struct smg_flow smg_flow;
typedef struct { double delta; int normalize; double stop_sphericity; } smg_flow_params;
enum { SMG_FLOW_SYSTEM = 0, SMG_FLOW_NORMALIZE = 1, SMG_FLOW_SPHERICITY = 2, SMG_FLOW_SPHERE = 3 };
smg_flow_params smg_flow_params_default(void);             /* 0.01, 1, 0.0 */
int smg_flow_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const smg_flow_params *p, smg_flow **out);
void smg_flow_destroy(smg_flow *f);
int smg_flow_set_params(smg_flow *f, const smg_flow_params *p);
int smg_flow_set_solver(smg_flow *f, int pcg);
long long smg_flow_device_bytes(const smg_flow *f);
int smg_flow_step(smg_flow *f, int n_steps, const smg_solve_opts *opts, double *sphericity_his, int *cycles, int *n_done);
int smg_flow_positions(smg_flow *f, int memspace, double *U, int ld_u);
int smg_flow_set_positions(smg_flow *f, const double *U, int ld_u, int memspace);
int smg_flow_reset(smg_flow *f);
int smg_flow_sphere(smg_flow *f, int memspace, double *S, int ld_s, double *sigma, double *stats);
int smg_flow_host(int op, int nV, int nF, const int *F, const double *U, const double *V0, const int *rowptr, const int *col, const double *L0,
                  double delta, double *out);

/* ---- Helmholtz-Hodge decomposition of per-face tangent vector fields (csrc/smg_hodge.cpp): Tong, Lombeyda, Hirani,
 * Desbrun 2003, with vertex potentials.  Per face f with vertices p0, p1, p2, unit normal n_f, area A_f, e_fi the edge opposite corner i and
 * W_fi = (n_f x e_fi) / (2 A_f) the gradient of vertex i's hat function (the basis of smg_geodesics, bit for bit), a field X_f (any 3-vector; only
 * its tangent part Xt_f = X_f - (X_f . n_f) n_f matters) is split as
 *     Xt = G + R + H,   G_f = sum_i u_i W_fi (grad u),   R_f = n_f x sum_i v_i W_fi (J grad v),   H = Xt - G - R
 * where u minimises sum_f A_f |Xt_f - grad u_f|^2, that is (-L) u = b with b_i = (1/2) sum (n_f x e_fi) . X_f, and v minimises
 * sum_f A_f |Xt_f - J grad v_f|^2, that is (-L) v = c with c_i = -(1/2) sum e_fi . X_f; both sums run over the corners (f, i) of the vertex, faces
 * ascending.  u: vertex 0 is known and 0.  v: on a closed mesh the same pin; on a mesh with boundary every boundary vertex is known and 0 and
 * nothing else.  With these constraints G, R and H are mutually orthogonal in the area inner product: |Xt|^2 = |G|^2 + |R|^2 + |H|^2.
 * smg_hodge_create: h gives the prolongations (any scalar hierarchy on this mesh, one level included); they are copied, h is not modified.
 *   A closed mesh gets ONE internal handle (-L, vertex 0 known), a mesh with boundary two (vertex 0 known; the boundary vertices known).
 *   SMG_ERR_INVALID, before any device work, for: a union or block hierarchy, nV that is not the hierarchy's level-0 rows, a face index out of
 *   range, a face of zero area, a non-finite coordinate, more than one connected component; then, for a mesh with boundary, no interior vertex.
 *   SMG_ERR_NO_DEVICE comes after all of them.  V: nV x 3 row-major, as every create takes it.
 * smg_hodge_set_solver: as smg_arap_set_solver (PCG by default).  smg_hodge_is_closed: 1 when no edge belongs to one face alone.
 * smg_hodge_decompose: X is k fields of nF x 3 row-major, field c at c * 3 nF (how smg_morph_reconstruct takes J); u and v are nV x k
 *   column-major with ld >= nV, rows past nV are left alone; parts (NULL ok) is k sets of nF x 9 row-major: G, R, H of the face; X, u, v and parts
 *   live in memspace.  energy (NULL ok, host) holds 4k doubles: sum A_f |Xt|^2, sum A_f |G|^2, sum A_f |R|^2, sum A_f |H|^2 per field, each a
 *   fixed-order sum.  cycles (NULL ok, host) holds 2 ints: the loop entries of the u solve and of the v solve.  On a closed mesh a call is ONE
 *   solve of 2k columns (b in columns 0 .. k - 1, c in k .. 2k - 1) and both entries carry its count; with boundary it is two k-column solves.
 *   The start is zero.  opts: the options of the solves (tol is absolute); NULL selects smg_solve_opts_default with max_iter = 100 and
 *   tol = 1e-10 |rhs|_F over the solve's columns (all rows, a fixed-order sum that the host reads once).  A non-finite norm returns
 *   SMG_ERR_NONFINITE before any solve, with nothing written to u, v, parts or energy.  A solve that used all of max_iter is not an error; a
 *   failing solve returns its code unchanged.  SMG_ERR_INVALID, before any device work, for: a null g, X, u or v; k < 1 (or k fields past the
 *   index range); a memspace that is neither SMG_HOST nor SMG_DEVICE; a leading dimension below nV.
 * smg_hodge_field: the inverse direction, X_f = grad u_f + J grad v_f for k pairs of potentials: one launch, no solve.  Refusals as above.
 * Nothing is allocated after create except the query blocks, which grow with the largest k seen and are kept (smg_hodge_device_bytes counts
 * them).  The same calls give the same bits, with graphs on or off and for SMG_HOST or SMG_DEVICE blocks.
 * smg_hodge_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with
 *   the operands and the layouts of smg_debug_hodge below.
 * Not covered: more than one boundary loop (v = 0 on all loops; the exact decomposition has one free constant per extra loop and the difference
 * lands in H), the non-conforming part of H (2 nF - 2 nV + 2 dimensions on a closed mesh, not only the 2g harmonic fields), per-vertex input
 * fields, union / block / sharded forms, moving meshes, an area-weighted zero mean for u. */
typedef struct smg_hodge smg_hodge;
enum { SMG_HODGE_RHS = 0, SMG_HODGE_PARTS = 1, SMG_HODGE_FIELD = 2 };
int smg_hodge_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, smg_hodge **out);
void smg_hodge_destroy(smg_hodge *g);
int smg_hodge_set_solver(smg_hodge *g, int pcg);
int smg_hodge_is_closed(const smg_hodge *g);
long long smg_hodge_device_bytes(const smg_hodge *g);
int smg_hodge_decompose(smg_hodge *g, const double *X, int k, int memspace, const smg_solve_opts *opts, double *u, int ld_u, double *v, int ld_v,
                        double *parts, double *energy, int *cycles);
int smg_hodge_field(smg_hodge *g, const double *u, int ld_u, const double *v, int ld_v, int k, int memspace, double *X);
int smg_hodge_host(int op, int nV, int nF, int k, const int *F, const double *V, const double *X, const double *u, const double *v, double *out);

/* ---- discrete conformal metrics with prescribed angle sums (csrc/smg_conformal.cpp): Springborn, Schroeder, Pinkall 2008,
 * "Conformal equivalence of triangle meshes".  One log scale factor u_i per vertex; the metric l~_ij = l_ij exp((u_i + u_j) / 2) is to have the
 * angle sum Theta_i at every free vertex.  The energy is convex, its gradient is g_i = (angle sum at i) - Theta_i and its Hessian half the
 * cotangent matrix of the current metric, so a Newton step is (-L~)_uu d = g_u, u += t d with -L~ assembled from the half cotangents of l~.
 * Every value of the matrix changes at every step and its pattern never: one full smg_precompute at create (-L of the rest mesh with the fixed
 * vertices known), then per Newton step one face kernel, one row kernel, smg_precompute_values_device and a 1-column solve from zero.
 *   The arithmetic: l0 = the rest length of the edge opposite every corner (nF x 3, index 3 f + c; the expressions of smg_mesh_cotmatrix);
 *   s_i = exp(-u_i / 2), the only exp; a face works with a_c = l0[3 f + c] s_{F[f][c]}, its lengths divided by the face's common factor, so no
 *   exp of a sum occurs.  With a, b, c the scaled lengths, S = a + b + c, s0 = b + c - a, s1 = a + c - b, s2 = a + b - c: the angle at corner 0 is
 *   2 atan2(sqrt(s1 s2), sqrt(S s0)) and its half cotangent (b b + c c - a a) / sqrt(S s0 s1 s2) / 2, cyclically; the quotient is formed as
 *   (b b + c c - a a) / (dA0 r) / 4 with dA0 twice the rest area (the cross product, as smg_mesh_cotmatrix has it) and r the ratio of
 *   sqrt(S s0 s1 s2) to the same root of the rest lengths, which is exactly 1 at u = 0: there -L~ is -smg_mesh_cotmatrix bit for bit.  A face with some s_c <= 0 is
 *   broken (Springborn's extension): the angle opposite the too-long edge is pi, the others 0, the half cotangents 0.  The angle sum of a vertex
 *   runs over its corner list, faces ascending; -L~ is summed in smg_mesh_cotmatrix's CSR order and term order.  No atomics, no FMA contraction.
 *   The line search is on the gradient norm: t = 1, 1/2, 1/4, ... is accepted when |g(u + t d)|_2 <= (1 - 1e-4 t) |g(u)|_2; below t = 2^-20 the
 *   call ends with SMG_OK, *converged = 0 and u the last accepted iterate.  The call stops when max |g_i| <= grad_tol or after max_newton steps.
 * smg_conformal_params: grad_tol (1e-10), max_newton (50), inner_rel_tol (1e-6: the inner solve's tol is inner_rel_tol |g|_2).
 * smg_conformal_create: h gives the prolongations (any scalar hierarchy on this mesh); they are copied into one internal handle, h is not
 *   modified.  fixed: the n_fixed vertices whose u is given, not solved for; they absorb whatever curvature remains (no Gauss-Bonnet test is
 *   made).  SMG_ERR_INVALID, before any device work, for: a union or block hierarchy, nV that is not the hierarchy's level-0 rows, a hierarchy
 *   of one level (smg_precompute_values_device needs two), a face index out of range, a face of zero area, a non-finite coordinate, more than
 *   one connected component; then an empty list, a fixed vertex out of range or listed twice, no free vertex; then grad_tol or inner_rel_tol
 *   not finite or <= 0, max_newton < 0.  SMG_ERR_NO_DEVICE comes after all of them.  V: nV x 3 row-major, as every create takes it.
 * smg_conformal_set_params: the parameters of the following calls.  smg_conformal_set_solver: as smg_arap_set_solver (PCG by default).
 * smg_conformal_solve: Theta (nV doubles; read at the free vertices) and u_fixed (n_fixed doubles in the order of create's list; NULL: zeros)
 *   live in memspace.  The call starts from the object's current u with the fixed entries set, so a second call is warm.  grad_his[t] = max |g|
 *   of iterate t (one entry more than *n_newton), step_his[t] = the accepted t, cycles[t] = the loop entries of the solve; all three, n_newton
 *   and converged may be NULL; the arrays hold max_newton (+ 1) entries.  opts: the options of the inner solves (tol is absolute and replaces
 *   inner_rel_tol |g|_2); NULL selects smg_solve_opts_default with that tol and max_iter = 100.  A solve that used all of max_iter is not an error; a failing
 *   precompute or solve returns its code unchanged.  A non-finite gradient norm returns SMG_ERR_NONFINITE with *n_newton = t, nothing written
 *   past grad_his[t] and u the last finite iterate (a trial with a non-finite norm is only a rejected trial).  SMG_ERR_INVALID, before any
 *   device work, for a null object or Theta, a bad memspace, and for SMG_HOST blocks a non-finite Theta or u_fixed (device blocks are not read
 *   by the host: there a non-finite entry ends as SMG_ERR_NONFINITE at step 0).  Per evaluation the host reads three doubles in one copy:
 *   sum g^2, max |g| and the number of broken faces.  Nothing is allocated after create.  The same calls give the same bits.
 * smg_conformal_reset: u = 0.  smg_conformal_set_u / smg_conformal_u: the state, nV doubles in memspace.
 * smg_conformal_angle_sums: the achieved angle sums of the current u at ALL nV vertices, the fixed ones included.
 * smg_conformal_lengths: l~ of the current u per corner (nF x 3, the edge opposite the corner) as l0 / (s_j s_k); what smg_mesh_unfold takes.
 * smg_conformal_stats: 2 host doubles: the broken faces of the last accepted iterate, and their maximum over every evaluation of the last solve.
 * smg_conformal_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with
 *   the operands and the layouts of smg_debug_conformal below.
 * Not covered: edge flips (Gu et al.: the metric stays on the given triangulation, so a broken face stays broken), a Gauss-Bonnet check of
 * Theta, hyperbolic or spherical background metrics, the energy itself (the line search needs only its gradient), union / block / sharded
 * forms, cutting a closed mesh into a disk for the layout. */
typedef struct smg_conformal smg_conformal;
typedef struct { double grad_tol; int max_newton; double inner_rel_tol; } smg_conformal_params;
enum { SMG_CONFORMAL_SCALE = 0, SMG_CONFORMAL_FACES = 1, SMG_CONFORMAL_ROWS = 2 };
smg_conformal_params smg_conformal_params_default(void);   /* 1e-10, 50, 1e-6 */
int smg_conformal_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const int *fixed, int n_fixed,
                         const smg_conformal_params *p, smg_conformal **out);
void smg_conformal_destroy(smg_conformal *c);
int smg_conformal_set_params(smg_conformal *c, const smg_conformal_params *p);
int smg_conformal_set_solver(smg_conformal *c, int pcg);
long long smg_conformal_device_bytes(const smg_conformal *c);
int smg_conformal_reset(smg_conformal *c);
int smg_conformal_set_u(smg_conformal *c, const double *u, int memspace);
int smg_conformal_u(smg_conformal *c, int memspace, double *u);
int smg_conformal_solve(smg_conformal *c, const double *Theta, const double *u_fixed, int memspace, const smg_solve_opts *opts, double *grad_his,
                        double *step_his, int *cycles, int *n_newton, int *converged);
int smg_conformal_angle_sums(smg_conformal *c, int memspace, double *sums);
int smg_conformal_lengths(smg_conformal *c, int memspace, double *len);
int smg_conformal_stats(const smg_conformal *c, double *stats);
int smg_conformal_host(int op, int nV, int nF, const int *F, const double *l0, const double *area2, const double *u, const double *d, double t,
                       const double *s, const double *Theta, const int *fixed, int n_fixed, double *out);

/* ---- Earth mover's (1-Wasserstein) distance between distributions on a mesh, with geodesic ground cost (csrc/smg_emd.cpp):
 * Solomon, Rustamov, Guibas, Butscher 2014 in Beckmann form.  With b = mu1 - mu0 (integrated masses per vertex, sum_i b_i = 0), A_f the face
 * areas and W2_fi the gradient of vertex i's hat function in the face's frame (t1 = (p1 - p0) / |p1 - p0|, t2 = n x t1):
 *     minimise  sum_f A_f |J_f|   subject to  sum_f A_f W2_fi . J_f = b_i for every vertex i;     dual: maximise b . psi, |grad psi_f| <= 1
 * by ADMM with one penalty rho_c = rho_scale sqrt(total area) / m_c per column (m_c = (1/2) sum_i |b_i|; 1 for a zero column), over-relaxation
 * alpha and the state Z, U (2 doubles each per face and column, zero at the start).  Iteration t: Y = Z - U; r_i = sum A_f W2_fi . Y_f - b_i;
 * (-L) phi = r with vertex 0 known and 0, ONE k-column solve warm-started from the previous phi with the absolute tolerance
 * inner_rel_tol |b|_F; J = Y - grad phi; T = alpha J + (1 - alpha) Z + U; Z = max(0, 1 - (1 / rho) / |T|) T; U = T - Z.  The bounds:
 * upper = sum_f A_f |J_f|; potential = (-rho / max(1, gmax)) phi with gmax = max_f rho |grad phi_f|, which is dual feasible whatever the
 * solve's accuracy; lower = b . potential.  A column is done when upper - lower <= gap_tol upper; the loop ends at an iteration that is a
 * multiple of check_every (or the last) at which every column is done, or at max_iter, which is not an error.  Between checks the host reads
 * nothing beside what the inner solve itself returns on every iteration (its history and its convergence flag); at a check it reads the 3 k
 * doubles of the bounds in one copy.  A query's fixed cost: the masses are brought to the host for the refusals, m_c and rho_c (SMG_DEVICE
 * blocks too: two copies of nV x k doubles down and b up again), DESIGN.md section 30 gives the figures.
 * smg_emd_create: h gives the prolongations (any scalar hierarchy on this mesh, one level included); they are copied, h is not modified.
 *   The checks of DESIGN.md section 21 in their order, with a connected mesh, then the parameters: gap_tol, rho_scale and inner_rel_tol finite
 *   and > 0, alpha inside (0, 2), max_iter >= 0, check_every >= 1; all SMG_ERR_INVALID before the device is touched.  Builds one cloned handle,
 *   precomputed once with -L and vertex 0 known.
 * smg_emd_solve: mu0, mu1 are nV x k column-major blocks (leading dimensions ld0, ld1 >= nV) in `memspace`; upper, lower and residual (k doubles
 *   each, host; residual may be NULL) and n_iter (host, may be NULL) are written; residual[c] = |weak divergence of J - b|_2 over the unknown
 *   rows of the last iteration, relative to |b_c|_2: the last solve's residual.  potential (NULL ok): nV x k in `memspace`, leading dimension
 *   ld_p >= nV.  flow (NULL ok): J of the last iteration as k x nF x 3 row-major in `memspace`, one extra launch.  warm != 0 continues from the
 *   kept Z, U, phi when k is the k of the previous call, otherwise the state is zeroed.  A column with b = 0 returns upper = lower = 0.
 *   max_iter = 0 writes upper = +infinity and lower = 0 for the non-zero columns.  opts (NULL: the defaults with the tolerance above and
 *   max_iter 100) are the inner solve's.  Refusals, SMG_ERR_INVALID before any launch: a null object or required block, k < 1, a bad memspace,
 *   a leading dimension below nV, a non-finite mass, a column with |sum_i b_i| > 1e-12 sum_i |b_i| ("masses differ").  A failing inner solve
 *   returns its code.
 * smg_emd_set_solver: as smg_arap_set_solver (PCG by default).  Nothing is allocated after create except the query blocks, which grow with
 *   the largest k seen and are kept (smg_emd_device_bytes counts them).
 * smg_emd_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with the
 *   operands and the layouts of smg_debug_emd below. */
typedef struct { double gap_tol; int max_iter; int check_every; double alpha, rho_scale, inner_rel_tol; } smg_emd_params;
enum { SMG_EMD_GEOMETRY = 0, SMG_EMD_RHS = 1, SMG_EMD_UPDATE = 2, SMG_EMD_DUAL = 3, SMG_EMD_FLOW = 4, SMG_EMD_RESIDUAL = 5 };
typedef struct smg_emd smg_emd;
smg_emd_params smg_emd_params_default(void);               /* 1e-2, 2000, 10, 1.7, 0.1, 1e-8 */
int smg_emd_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const smg_emd_params *p, smg_emd **out);
void smg_emd_destroy(smg_emd *g);
int smg_emd_set_params(smg_emd *g, const smg_emd_params *p);
int smg_emd_set_solver(smg_emd *g, int pcg);
long long smg_emd_device_bytes(const smg_emd *g);
int smg_emd_solve(smg_emd *g, const double *mu0, int ld0, const double *mu1, int ld1, int k, int memspace, const smg_solve_opts *opts, int warm,
                  double *upper, double *lower, int *n_iter, double *residual, double *potential, int ld_p, double *flow);
int smg_emd_host(int op, int nV, int nF, int k, const int *F, const double *V, const double *b, const double *phi, const double *state,
                 const double *rho, double alpha, double *out);

/* ---- Incompressible flow on a surface in vorticity - stream-function form (csrc/smg_fluid.cpp): the state is the
 * vorticity w, one double per (vertex, column), resident on the device; k columns are k independent simulations and k columns of every solve.
 * With -L the positive semi-definite cotangent matrix and m_i the barycentric mass (a third of the areas around i):
 *     (-L) psi = -m (w - wbar),    u_f = n_f x grad psi_f,    dw/dt + u . grad w = viscosity Laplace w
 * Closed mesh: wbar_c = sum(m w_c) / sum(m) (fixed-order sums) and vertex 0 is known and 0.  Mesh with boundary: wbar = 0 and every boundary
 * vertex is known and 0, so the boundary is a streamline.  Transport is a finite-volume scheme on the barycentric dual cells: in face (i, j, k),
 * counter-clockwise, with c = (psi_i + psi_j + psi_k) / 3 the flux out of i's cell into j's is Phi_ij = (psi_i + psi_j) / 2 - c and into k's
 * Phi_ik = c - (psi_i + psi_k) / 2 -- no geometry is read;
 *     adv_i = -(1 / m_i) sum_segments (1/2) (Phi - theta |Phi|) (w_nbr - w_i),      rate_i = (1 / m_i) sum_segments max(Phi, 0)
 * summed in corner-list order (faces ascending, ij before ik); theta = 1 is first-order upwind, 0 the central flux.  Time stepping is SSP
 * Runge-Kutta in Shu-Osher form: every stage is out = a w_n + b (w_s + dt adv(w_s)) with its own psi_s, (a, b) = (0, 1) | (0, 1), (1/2, 1/2) |
 * (0, 1), (3/4, 1/4), (1/3, 2/3) for stages = 1 | 2 | 3; every solve is warm-started from the previous stage's psi.  dt > 0 is the fixed step;
 * dt == 0 takes dt_c = cfl / max_i rate_i of the step's first stage per column, formed on the device (no host read).  A step's reported cfl is
 * dt_c times the maximum over its stages of max_i rate_i.  viscosity > 0 (needs dt > 0): after the stages (M + viscosity dt (-L)) w_new = m w*
 * on a second handle without known rows -- the natural boundary condition for w, NOT a no-slip wall -- precomputed at create and by values
 * again when set_params changes viscosity dt.  Between two stages the host reads one double, |rhs|_F^2: it sets the default tolerance
 * (opts NULL: 1e-10 |rhs|_F, max_iter 100, per solve) and refuses non-finite input.
 * smg_fluid_create: h gives the prolongations (any scalar hierarchy on this mesh; one level is accepted when viscosity == 0); they are copied,
 *   h is not modified.  The checks of DESIGN.md section 21 in their order with a connected mesh, then "no interior vertex", then the parameters:
 *   theta finite and inside [0, 1], stages in 1..3, viscosity >= 0 (not NaN), dt >= 0, viscosity > 0 needs dt > 0, dt == 0 needs cfl > 0; all
 *   SMG_ERR_INVALID before the device is touched.
 * smg_fluid_set_params: the same parameter checks; changing between zero and non-zero viscosity is refused.
 * smg_fluid_set_vorticity: w is nV x k column-major (leading dimension ld >= nV) in `memspace`; sets k, zeroes psi and the times.
 * smg_fluid_vorticity: the state into w (nV x k, leading dimension ld, in `memspace`).
 * smg_fluid_step: n_steps steps.  cfl_his and time (n_steps x k row-major, host, NULL ok): every step's cfl and the time after it; cycles
 *   (n_steps, host, NULL ok): the loop entries of the step's solves, summed; n_done (host, NULL ok): the completed steps.  A non-finite
 *   right-hand side ends the call with SMG_ERR_NONFINITE: the state and the times of the last completed step are kept and the histories hold
 *   n_done rows.  A solve that does not reach its tolerance is not an error.
 * smg_fluid_stream: solves for the current state (warm-started; the result is kept as the next warm start) and writes psi (nV x k, leading
 *   dimension ld) in `memspace`.  smg_fluid_velocity: the same solve, then U = n x grad psi as k x nF x 3 row-major in `memspace`.
 * smg_fluid_diagnostics: the same solve, then out (host, 4 k: four rows of k) = circulation sum m w, enstrophy (1/2) sum m w^2, energy
 *   (1/2) sum A_f |grad psi_f|^2, and wbar as the solve uses it.
 * Call refusals, SMG_ERR_INVALID before any launch: a null object or block, k < 1, a bad memspace, a leading dimension below nV, a call before
 *   smg_fluid_set_vorticity, n_steps < 1.
 * smg_fluid_set_solver: as smg_arap_set_solver (PCG by default).  smg_fluid_is_closed: 1 when no edge belongs to one face alone.  Nothing is
 *   allocated after create except the state's blocks, which grow with the largest k seen and are kept, and the histories of the longest call
 *   (smg_fluid_device_bytes counts them).
 * smg_fluid_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with the
 *   operands and the layouts of smg_debug_fluid below. */
typedef struct { double theta; int stages; double viscosity, dt, cfl; } smg_fluid_params;
enum { SMG_FLUID_RHS = 0, SMG_FLUID_ADVECT = 1, SMG_FLUID_VELOCITY = 2, SMG_FLUID_DIAG = 3, SMG_FLUID_DT = 4 };
typedef struct smg_fluid smg_fluid;
smg_fluid_params smg_fluid_params_default(void);           /* 0.0, 3, 0.0, 0.0, 0.5 */
int smg_fluid_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const smg_fluid_params *p, smg_fluid **out);
void smg_fluid_destroy(smg_fluid *g);
int smg_fluid_set_params(smg_fluid *g, const smg_fluid_params *p);
int smg_fluid_set_solver(smg_fluid *g, int pcg);
int smg_fluid_is_closed(const smg_fluid *g);
long long smg_fluid_device_bytes(const smg_fluid *g);
int smg_fluid_set_vorticity(smg_fluid *g, const double *w, int ld, int k, int memspace);
int smg_fluid_vorticity(smg_fluid *g, double *w, int ld, int memspace);
int smg_fluid_step(smg_fluid *g, int n_steps, const smg_solve_opts *opts, double *cfl_his, double *time, int *cycles, int *n_done);
int smg_fluid_stream(smg_fluid *g, const smg_solve_opts *opts, double *psi, int ld, int memspace);
int smg_fluid_velocity(smg_fluid *g, const smg_solve_opts *opts, double *U, int memspace);
int smg_fluid_diagnostics(smg_fluid *g, const smg_solve_opts *opts, double *out);
int smg_fluid_host(int op, int nV, int nF, int k, const int *F, const double *V, const double *w, const double *psi, const double *wn, double a,
                   double b, const double *dt, double theta, int rates_only, double *out);

/* ---- Two-species reaction-diffusion on a surface (csrc/smg_rd.cpp): the state is the pair (u, v), two doubles per
 * (vertex, column), resident on the device; k columns are k independent simulations with their own reactions and k (or 2k) columns of every
 * solve.  With -L the positive semi-definite cotangent matrix and m_i the barycentric mass (a third of the areas around i), per column c
 *     u_t = Du Laplace u + R_u(u, v; c),    v_t = Dv Laplace v + R_v(u, v; c)
 * with the natural (no-flux) boundary condition: no row is known, on closed and on open meshes.  R_u and R_v are bivariate cubics over the
 * monomials 1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3 in this order: 20 doubles per column, R_u's ten first (the table `coeff`, k x 20
 * row-major).  A step is IMEX: the reaction explicit, the diffusion implicit.
 *   1. k_rd_react: (u, v) through react_substeps Euler steps of length dt / react_substeps of the reaction alone (both rates from the same
 *      (u, v)), giving (u*, v*); the right-hand sides m u*, m v* and their squares.
 *   2. (M + dt Du (-L)) u' = m u*, (M + dt Dv (-L)) v' = m v*, warm-started from (u, v).  Du != Dv, Dv > 0: a k-column solve on each of two
 *      handles.  Du == Dv: ONE 2k-column solve on one handle.  Dv == 0: v' = v* from the kernel, bit for bit, and one k-column solve.
 *   3. k_rd_close: the terms m u', m v' and max(|u' - u|, |v' - v|); fixed-order sums and maxima per column.
 * The matrices are precomputed at create and by values again when set_params changes dt Du or dt Dv.  The host reads per step |m u*|_F^2 and
 * |m v*|_F^2 before the solves -- they set the default tolerance (opts NULL: 1e-10 |rhs|_F of the solve's own columns, max_iter 100) and
 * refuse non-finite input -- and the 3k sums and maxima after them.  A step writes into the block beside the state and commits by an index
 * swap, so a refused step leaves the state of the last completed one.
 * smg_rd_create: h gives the prolongations (any scalar hierarchy on this mesh, at least two levels); they are copied, h is not modified.  The
 *   checks, all SMG_ERR_INVALID before the device is touched, in this order: a null argument; a union or block hierarchy; nV not the level-0
 *   rows; fewer than two levels; the mesh (indices, areas, finite coordinates, one component); then the parameters in their order: Du finite
 *   and > 0, Dv finite and >= 0, dt finite and > 0, react_substeps >= 1, stop_change >= 0 (not NaN).  SMG_ERR_NO_DEVICE after all of them.
 * smg_rd_set_params: the same parameter checks; a change between the three cases of handle use (Du != Dv with Dv > 0 | Du == Dv | Dv == 0)
 *   is refused.
 * smg_rd_set_state: u, v are nV x k column-major (leading dimension ld >= nV) in `memspace`; coeff is k x 20 row-major on the HOST, every
 *   entry finite; sets k.
 * smg_rd_state: the state into u, v (nV x k each, leading dimension ld, in `memspace`).
 * smg_rd_step: at most n_steps steps.  mass_his (n_steps x 2k row-major: sum m u per column, then sum m v), change_his (n_steps x k: max_i
 *   max(|u' - u|, |v' - v|)), cycles (n_steps x 2: the loop entries of the first and of the second solve, 0 where there is none), n_done: host,
 *   NULL ok.  The loop ends after a step whose change is <= stop_change in every column (stop_change == 0: never early).  A non-finite
 *   right-hand side ends the call with SMG_ERR_NONFINITE: the state of the last completed step is kept and the histories hold n_done rows.  A
 *   solve that does not reach its tolerance is not an error.
 * Call refusals, SMG_ERR_INVALID before any launch: a null object or block, k < 1, a bad memspace, a leading dimension below nV, a non-finite
 *   coefficient, a call before smg_rd_set_state, n_steps < 1.
 * smg_rd_set_solver: as smg_arap_set_solver (PCG by default).  Nothing is allocated after create except the state's blocks, which grow with
 *   the largest k seen and are kept (smg_rd_device_bytes counts them).
 * smg_rd_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with the
 *   operands and the layouts of smg_debug_rd below. */
typedef struct { double Du, Dv, dt; int react_substeps; double stop_change; } smg_rd_params;
enum { SMG_RD_REACT = 0, SMG_RD_CLOSE = 1 };
typedef struct smg_rd smg_rd;
smg_rd_params smg_rd_params_default(void);                 /* 1.0, 1.0, 1.0, 1, 0.0 */
int smg_rd_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const smg_rd_params *p, smg_rd **out);
void smg_rd_destroy(smg_rd *g);
int smg_rd_set_params(smg_rd *g, const smg_rd_params *p);
int smg_rd_set_solver(smg_rd *g, int pcg);
long long smg_rd_device_bytes(const smg_rd *g);
int smg_rd_set_state(smg_rd *g, const double *u, const double *v, int ld, int k, const double *coeff, int memspace);
int smg_rd_state(smg_rd *g, double *u, double *v, int ld, int memspace);
int smg_rd_step(smg_rd *g, int n_steps, const smg_solve_opts *opts, double *mass_his, double *change_his, int *cycles, int *n_done);
int smg_rd_host(int op, int nV, int nF, int k, const int *F, const double *V, const double *u, const double *v, const double *coeff, double dt,
                int substeps, const double *un, const double *vn, double *out);

/* ---- Heat-kernel optimal transport on a mesh, the host side (csrc/smg_sinkhorn.cpp; Solomon et al. 2015, Convolutional
 * Wasserstein Distances): the pointwise operations of Sinkhorn iterations whose only non-pointwise operation is the heat kernel, on caller
 * arrays, with no GPU.  Mass form, as smg_emd: m_i the barycentric vertex mass (the expression of k_fluid_mass), A = sum m in the order of the
 * fixed-order sums; distributions are integrated masses per vertex.  With y = K(r) the output of a kernel application to the block r and sr_c the
 * fixed-order sum of r's column c,
 *     y_eff = max(y, 0) + (floor sr_c) / A
 * a uniform rank-one part that keeps the kernel symmetric and strictly positive where a solve's tail is below its accuracy.
 * F: nF x 3; V: nV x 3 row-major; blocks are column-major with leading dimension nV; planes are planes of nV; every sum is a fixed-order sum.
 *   SMG_SINKHORN_SCALE    y, r (nV x k), mu (nV x k_in: column c reads mu's column c % k_in), sr (k), floor -> out = r' = mu / y_eff (0 where
 *                         mu == 0; nV x k), the planes |r y_eff - mu| and r'^2 (k planes each), sum r' (k), the errors' sums (k), the squares' sum (1)
 *   SMG_SINKHORN_SUBSTEP  y (nV x k) -> out = m y (nV x k), its squares (k planes), their sum (1)
 *   SMG_SINKHORN_VALUE    r = r_v, y = r_w, mu = mu0, mu1 (nV x k each) -> out = the terms mu0 ln(r_v / m) + mu1 ln(r_w / m), a product with a zero
 *                         mass left out (k planes), ln v, ln w (nV x k each; -inf where the mass is 0), the terms' sums (k)
 *   SMG_SINKHORN_GEOMEAN  k = G groups of k_in columns: y = z, r = r_v (nV x G k_in), mu = the previous masses (nV x G), sr (G k_in), alphas (G x k_in
 *                         row-major), floor; per column d_c = (r_v,c / m) z_eff,c, mu = exp(sum_c alpha_c ln d_c) over the columns with alpha_c > 0
 *                         (0 where such a d_c is not > 0) -> out = r_v' = m mu / z_eff (nV x G k_in), the masses m mu (nV x G), |m mu - previous| (G
 *                         planes), r_v'^2 (G k_in planes), sum r_v' (G k_in), the changes' sums (G), the masses' sums (G), the squares' sum (1)
 * SMG_ERR_INVALID, in this order, for an unknown op, nV < 1, nF < 1, F, V or out missing; a missing operand; k < 1; for the scale and the
 * geomean k_in < 1, then a floor that is not finite and >= 0; a face index out of range. */
enum { SMG_SINKHORN_SCALE = 0, SMG_SINKHORN_SUBSTEP = 1, SMG_SINKHORN_VALUE = 2, SMG_SINKHORN_GEOMEAN = 3 };
int smg_sinkhorn_host(int op, int nV, int nF, int k, int k_in, const int *F, const double *V, const double *y, const double *r, const double *mu,
                      const double *mu1, const double *sr, const double *alphas, double floor, double *out);

/* ---- The wave equation on a surface, with shots and receivers (csrc/smg_wave.cpp): the state is the pair (u, v = u_t), two
 * doubles per (vertex, column), resident on the device; k columns are k independent experiments ("shots") and k columns of every solve.  With
 * C = -L the positive semi-definite cotangent matrix, m_i the barycentric mass (a third of the areas around i), mt_i = m_i / speed_i^2,
 * sigma_i >= 0 a damping rate per vertex and f(t) integrated nodal forces, per column
 *     Mt u_tt + Sigma Mt u_t + C u = f(t),      Mt = diag(mt_i), Sigma = diag(sigma_i)
 * stepped by the trapezoidal rule in (u, v) (Newmark with beta = 1/4, gamma = 1/2).  With s2_i = 2.0 + sigma_i * dt, a = 0.25 * dt * dt,
 * q2 = 2.0 / dt (host doubles, formed once) and w = u + u':
 *   1. k_wave_rhs: b_i = mt_i * (s2_i * u_i + dt * v_i), its squares (0.0 on a known row) and the warm start 2.0 * u + dt * v.  Within a call
 *      and across calls the previous step's k_wave_advance has already left all three: only the first step after set_state or set_params runs
 *      this kernel.
 *   2. k_wave_sources (a signal is given): b_i += a * (f_i(t_n) + f_i(t_n+1)) at the source vertices, the squares rewritten there.
 *   3. A w = b,  A = diag(0.5 * s2_i * mt_i) + a C, warm-started from 2u + dt v, which the kernels write into the block the solve returns w in
 *      (smg_solve and smg_solve_pcg gather z0 into the handle before they scatter z).
 *   4. k_wave_advance: u' = w - u, v' = q2 * (u' - u) - v, the kinetic terms 0.5 * ((mt_i * v') * v'), and the next step's b, squares and warm
 *      start from (u', v') with k_wave_rhs's expressions; the potential energy 0.5 u' C u' is the sum of k_fluid_velocity's face terms of u'.
 *   5. k_wave_record: u' at the receivers into row t of the trace buffer.
 * No product with C is needed.  A is precomputed at create and by values again when set_params changes dt or damping.  The host reads per step
 * |b|_F^2 before the solve -- it sets the default tolerance (opts NULL: 1e-10 |b|_F, max_iter 100) and refuses non-finite input -- and, where
 * energy_his is given, the 2k energy sums after it.  A step writes into the block beside the state and commits by an index swap, so a refused
 * step leaves the state of the last completed one.
 * Boundary: clamped = 0 is the natural (free) boundary, no row is known, on closed and on open meshes; clamped = 1 makes the boundary vertices
 *   known rows of the handle with value 0: u, v and forces on those rows must be 0, and the kernels then return exact zeros there.
 * smg_wave_create: h gives the prolongations (any scalar hierarchy on this mesh, at least two levels); they are copied, h is not modified.
 *   speed: nV doubles, finite and > 0, NULL: 1 everywhere; sigma: nV doubles, finite and >= 0, NULL: p->damping everywhere.  The checks, all
 *   SMG_ERR_INVALID before the device is touched, in this order: a null argument; a union or block hierarchy; nV not the level-0 rows; fewer
 *   than two levels; the mesh (indices, areas, finite coordinates, one component); the parameters in their order: dt finite and > 0, damping
 *   finite and >= 0, clamped 0 or 1; speed; sigma; then for clamped = 1 a mesh without boundary and a mesh without interior vertex.
 *   SMG_ERR_NO_DEVICE after all of them.
 * smg_wave_set_params: the same parameter checks; a new dt or damping (damping counts only where sigma was NULL) rebuilds s2, a, q2 and
 *   re-precomputes by values; a change of clamped is refused.  The kept right-hand side is dropped.
 * smg_wave_set_state: u, v are nV x k column-major (leading dimension ld >= nV) in `memspace`; sets k.  When clamped, a u or v that is not 0
 *   on a boundary row is refused (one small kernel and one host read) and the object is left without a state.
 * smg_wave_state: the state into u, v (nV x k each, leading dimension ld, in `memspace`).
 * smg_wave_set_sources: any time after create; n_src >= 0 vertices in range, none twice (so the source kernel writes without atomics), none on
 *   a clamped boundary vertex.  smg_wave_set_receivers: n_rec >= 0 vertices in range; duplicates are allowed.
 * smg_wave_step: at most n_steps steps.  signal (host, NULL: no force): (n_steps + 1) x n_src x k row-major, entry [t][j][c] the nodal force at
 *   source j in column c at the call's start time plus t dt; with n_src == 0 or a non-finite entry it is refused; uploaded once per call.
 *   energy_his (n_steps x 2k row-major: kinetic then potential energy per column, after each step; NULL: the potential-energy launches and
 *   the read are skipped), traces (n_steps x n_rec x k: u' at the receivers after each step, gathered on the device and copied once at the
 *   end of the call; NULL or n_rec == 0: skipped), cycles (n_steps: the loop entries of each solve), n_done: host, NULL ok.  A non-finite
 *   right-hand side ends the call with SMG_ERR_NONFINITE: the state of the last completed step is kept and the histories hold n_done rows.
 *   A solve that does not reach its tolerance is not an error.
 * Call refusals, SMG_ERR_INVALID before any launch: a null object or block, k < 1, k columns beyond the index range, a bad memspace, a leading
 *   dimension below nV, a bad list, a call before smg_wave_set_state, n_steps < 1, a bad signal.
 * smg_wave_set_solver: as smg_arap_set_solver (PCG by default).  Nothing is allocated after create except the blocks that grow with the largest
 *   k, n_steps, n_src and n_rec seen and are kept (smg_wave_device_bytes counts them).
 * smg_wave_host: the host twin of the kernels on caller arrays (no GPU, the text the kernels compile, the sums in the device's order), with the
 *   operands and the layouts of smg_debug_wave below. */
typedef struct { double dt, damping; int clamped; } smg_wave_params;
enum { SMG_WAVE_RHS = 0, SMG_WAVE_SOURCES = 1, SMG_WAVE_ADVANCE = 2, SMG_WAVE_RECORD = 3 };
typedef struct smg_wave smg_wave;
smg_wave_params smg_wave_params_default(void);             /* 1.0, 0.0, 0 */
int smg_wave_create(const smg_hierarchy *h, const double *V, int nV, const int *F, int nF, const double *speed, const double *sigma,
                    const smg_wave_params *p, smg_wave **out);
void smg_wave_destroy(smg_wave *g);
int smg_wave_set_params(smg_wave *g, const smg_wave_params *p);
int smg_wave_set_solver(smg_wave *g, int pcg);
long long smg_wave_device_bytes(const smg_wave *g);
int smg_wave_set_state(smg_wave *g, const double *u, const double *v, int ld, int k, int memspace);
int smg_wave_state(smg_wave *g, double *u, double *v, int ld, int memspace);
int smg_wave_set_sources(smg_wave *g, const int *idx, int n_src);
int smg_wave_set_receivers(smg_wave *g, const int *idx, int n_rec);
int smg_wave_step(smg_wave *g, int n_steps, const double *signal, const smg_solve_opts *opts, double *energy_his, double *traces, int *cycles,
                  int *n_done);
int smg_wave_host(int op, int nV, int nF, int k, const int *F, const double *V, const double *speed, const double *sigma, int clamped, double dt,
                  const double *u, const double *v, const double *w, const int *idx, int n_idx, const double *sig0, const double *sig1, double *out);

/* ---- Adjoint-state gradients of a trace misfit through the wave object's own time stepper (csrc/smg_wave_adjoint.cpp).
 * With rho_n = R u_n - observed_n (R gathers u at the receivers; a duplicated receiver counts once per slot) the misfit of column c is
 *     J_c = 0.5 * sum_{n = 1 .. N} sum_r rho_{n,r,c}^2
 * and smg_wave_gradient differentiates it exactly -- the discrete adjoint of the scheme above, not of the differential equation -- with respect
 * to the speed, the state (u_0, v_0) the call starts from and the signal.  A = diag(0.5 * s2 * mt) + a C is symmetric, so the transposed step
 * is ONE solve of the same precomputed matrix on the same handle between pointwise kernels; k shots stay k columns:
 *   forward, step n = 0 .. N - 1: smg_wave_step's launches, then k_wave_adj_keep: e_n = dt * v_n - (0.5 * s2) * (u_{n+1} - u_n), one nV x k block.
 *   k_wave_adj_residual: rho = traces - observed and its squares in k planes; J_c = 0.5 * their fixed-order sum.
 *   backward from p = R' rho_N, q = 0, Y = 0, G = 0; for n = N - 1 .. 0:
 *     1. k_wave_adj_rhs: g = p + q2 * q and its squares, both 0.0 on a known row.
 *     2. A y = g, warm-started from the y of step n + 1; the host reads |g|_F^2 as the forward step reads |b|_F^2 (opts NULL: 1e-10 |g|_F, max_iter
 *        100).  |g|_F^2 == 0.0: the solve is skipped, y = 0 and the step's cycles entry is 0.
 *     3. k_wave_adj_advance: G += y * e_n, t = mt * y, p = (s2 * t - p) - (2.0 * q2) * q, q = dt * t - q (both from the old p and q).
 *     4. k_wave_adj_signal (grad_signal wanted): gs[n] += a * y[src], gs[n + 1] += a * y[src].
 *     5. k_wave_adj_inject (n >= 1): p += R' rho_n.  The receivers are grouped by vertex at the first call after smg_wave_set_receivers: one lane
 *        owns a vertex and adds its slots in ascending slot order, without atomics.  A receiver on a clamped row contributes nothing.
 *   k_wave_adj_scale: grad_speed = ((-2.0 * mt) / speed) * G, the factor a host plane formed once, as mt is.
 * On clamped rows y, p, q and G are exact zeros.
 * smg_wave_gradient: runs n_steps steps from the current state.  signal, opts, traces, n_done: as smg_wave_step; the forward half leaves the state
 *   and the traces that smg_wave_step with the same arguments would leave, bit for bit: the state afterwards is (u_N, v_N).  observed (host, NULL:
 *   zeros): n_steps x n_rec x k, the layout of traces.  Outputs, host, each NULL ok: misfit (k); grad_speed (nV x k column-major, leading dimension
 *   ld: one gradient per shot, the caller sums them); grad_u0, grad_v0 (nV x k, leading dimension ld0); grad_signal ((n_steps + 1) x n_src x k);
 *   cycles (2 * n_steps: the forward solves' loop entries in step order, then the backward solves' in the order they ran, entry n_steps + j of
 *   step n_steps - 1 - j).  With every gradient output NULL the backward pass is skipped and nothing is kept.
 *   Refusals, SMG_ERR_INVALID before any launch, in this order: a null object; no state; n_steps < 1; no receivers; a signal without sources or with
 *   a non-finite entry; n_steps x n_rec x k beyond the index range; a non-finite observed entry; a leading dimension below nV; grad_signal without a
 *   signal.  A forward step that is refused ends the call as it ends smg_wave_step: the state of the last completed step, *n_done, and neither
 *   misfit nor gradient written.  A non-finite |g|_F^2 ends the call with SMG_ERR_NONFINITE: the state is (u_N, v_N), no gradient is written.
 *   The adjoint right-hand side uses the forward step's blocks, so the kept right-hand side is dropped: the next smg_wave_step forms it again,
 *   to the same bits.
 *   Memory: allocated at the first call, grown with the largest shape seen, kept, counted by smg_wave_device_bytes: the history, n_steps x nV x k
 *   doubles (at 1 M vertices -- the 1 011 330 of the benchmark's mesh -- k = 8 and 100 steps it is 6.5 GB; there is no checkpointing, so a longer
 *   run needs fewer columns per call); p, q, y, G (nV x k each); the residuals, their squares and the observed traces (3 x n_steps x n_rec x k); the grouped
 *   receiver list; the signal's gradient; the factor plane.
 * smg_wave_set_speed: a new speed for the following steps (nV doubles, finite and > 0 -- create's check and message; NULL: 1 everywhere): rebuilds
 *   mt from the masses kept on the host and re-precomputes by values; the kept right-hand side is dropped.  The state is kept.
 * smg_wave_adjoint_host: the host twin of the new kernels on caller arrays (no GPU), with the operands and layouts of smg_debug_wave_adjoint. */
enum { SMG_WAVE_ADJ_KEEP = 0, SMG_WAVE_ADJ_RESIDUAL = 1, SMG_WAVE_ADJ_INJECT = 2, SMG_WAVE_ADJ_RHS = 3, SMG_WAVE_ADJ_ADVANCE = 4, SMG_WAVE_ADJ_SIGNAL = 5,
       SMG_WAVE_ADJ_SCALE = 6 };
int smg_wave_gradient(smg_wave *g, int n_steps, const double *signal, const double *observed, const smg_solve_opts *opts, double *misfit,
                      double *grad_speed, int ld, double *grad_u0, double *grad_v0, int ld0, double *grad_signal, double *traces, int *cycles,
                      int *n_done);
int smg_wave_set_speed(smg_wave *g, const double *speed);
int smg_wave_adjoint_host(int op, int nV, int nF, int k, const int *F, const double *V, const double *speed, const double *sigma, int clamped, double dt,
                          const double *x0, const double *x1, const double *x2, const double *x3, const double *x4, const int *idx, int n_idx, int n_rows,
                          double *out);

/* ---- Born traces and Gauss-Newton products of the trace misfit (csrc/smg_wave_born.cpp).  With J = d traces / d speed,
 * smg_wave_gauss_newton returns the linearised (Born) traces J d and the Gauss-Newton product H d = J' J d that truncated-Newton inversion
 * (Gauss-Newton with conjugate gradients) is built on.  A speed perturbation d changes mt by fd = fac * d, fac = (-2.0 * mt) / speed the plane
 * k_wave_adj_scale reads, and the right-hand side of step n by fd * e_n, e_n the block smg_wave_gradient keeps: the tangent run is the forward
 * step itself from the zero state, without nodal sources, with one distributed source per step; J d is its traces.  The adjoint pass is linear
 * in its residual and its coefficients do not depend on it: run with rho = J d it leaves J' J d in the place of grad_speed.  Hence
 * <d, H d> = |J d|^2 per column and <w, H d> = <J w, J d>.
 * Linearisation point: the run of the last smg_wave_gradient call that completed with a backward pass (a gradient output was given): its
 *   n_steps = N, its k columns, its kept history.  The object records it as valid at the end of such a call.  smg_wave_set_speed,
 *   smg_wave_set_params, smg_wave_set_receivers, a smg_wave_set_state that changes k and a gradient call with a backward pass that fails after its
 *   forward half has begun drop it; smg_wave_step, smg_wave_set_sources, a smg_wave_set_state with the same k and a gradient call without a backward
 *   pass (it does not write the history) keep it.
 * The call: fd formed on the host, one multiply per entry, uploaded once.  The tangent run, step n = 0 .. N - 1 on two state blocks of its own:
 *     1. k_wave_rhs where the previous k_wave_advance has not left the right-hand side (the first step runs it on the zeroed state).
 *     2. k_wave_born: off the known rows b = b + fd[i, c % d_cols] * e_n[i, c] and its square; a known row keeps its 0.0.
 *     3. the fixed-order sum and the host's read of |b|_F^2: non-finite refuses; exactly 0.0 (d == 0) skips the solve with w = 0 and a cycles
 *        entry of 0; otherwise opts NULL is 1e-10 |b|_F, max_iter 100.
 *     4. the solve, warm-started from 2 * du + dt * dv.   5. k_wave_advance.   6. k_wave_record.
 *   No energies, no sources, no k_wave_adj_keep.  Then k_wave_adj_residual of the Born traces without an observed block and k fixed-order
 *   sums (curvature); then, where product is wanted, smg_wave_gradient's backward loop without the signal's gradient, k_wave_adj_scale and the copy.
 * d: host, nV x d_cols column-major, leading dimension ldd, d_cols 1 or k; column c reads column c % d_cols, so one direction serves every shot.
 * Outputs, host, each NULL ok but not all three: product (nV x k, leading dimension ld: one H d per shot, the caller sums them as with grad_speed;
 *   exact zeros on clamped rows; NULL: the backward pass is skipped -- Born modelling alone, one forward run's cost); born_traces (N x n_rec x k, the
 *   layout of traces); curvature (k: |J d|^2 per column, the fixed-order sum of the squares of the returned born_traces, bit for bit); cycles (2 N,
 *   NULL ok: the tangent solves in step order, then the backward solves in the order they ran; N entries are written where product is NULL).
 * The object's state (u, v) is not touched.  The kept right-hand side is dropped, as the gradient call drops it; the next smg_wave_step forms it
 *   again, to the same bits.
 * Refusals, SMG_ERR_INVALID before any launch, in this order: a null object; no linearisation point; d missing; d_cols not 1 or k; ldd < nV; a
 *   non-finite entry of d; every output NULL; product with ld < nV.  A non-finite right-hand side in either half ends the call with
 *   SMG_ERR_NONFINITE and nothing written; the linearisation point is kept.
 * Memory: two tangent state blocks (nV x 2k each) and the plane fd (nV x d_cols), allocated at the first call, grown with the largest shape
 *   seen, kept, counted by smg_wave_device_bytes; everything else is the gradient call's.
 * smg_wave_born_host: the host twin of k_wave_born on caller arrays (no GPU), with the operands and layouts of smg_debug_wave_born. */
int smg_wave_gauss_newton(smg_wave *g, const double *d, int ldd, int d_cols, const smg_solve_opts *opts, double *product, int ld,
                          double *born_traces, double *curvature, int *cycles);
int smg_wave_born_host(int nV, int nF, int k, int d_cols, const int *F, int clamped, const double *b, const double *e, const double *fd, double *out);

/* Split-phase form of the same loop for column-sharded multi-GPU runs: the caller owns
 * the all-reduce of the residual sum of squares between the two halves of an iteration.
 *   begin:     gathers RHS/z0 (column-major) into the handle, resets the control block.  SMG_DEVICE: the gathers are ENQUEUED on the
 *              handle's stream and the call returns (stream-ordered, like every other entry point of the split-phase API: do not
 *              overwrite RHS / z0 from another stream before that work has run); SMG_HOST: the host blocks are consumed on return;
 *   residual:  *d_sumsq (device double) = sum over the local columns of |RHS_u - A_0 z_u|^2   (.cpp:110/:332);
 *   cycle:     r = sqrt(*d_sumsq) -> r_his, break test, then one V-cycle (skipped on the device once done);
 *   end:       scatters z, copies r_his back, reports convergence.
 * residual and cycle run as cached graphs that write / read *d_sumsq in place (no staging copy): hand the SAME device buffer to
 * both, every iteration (another buffer is honoured, at the price of re-capturing the two graphs).  NULL = the handle's own word. */
int smg_solve_begin(smg_hierarchy *h, const double *RHS, int ld_rhs, const double *known_val, int ld_kv,
                    const double *z0, int ld_z0, int k, int memspace, const smg_solve_opts *opts);
int smg_solve_iter_residual(smg_hierarchy *h, double *d_sumsq);
int smg_solve_iter_cycle(smg_hierarchy *h, const double *d_sumsq);
/* Latency-hiding form of `cycle`: the V-cycle of iteration i does not wait for the all-reduce of residual i.
 *   cycle_speculative:  saves the iterate, runs the V-cycle in place (independent of the pending reduction);
 *   commit(d_sumsq):    r = sqrt(*d_sumsq) -> r_his, break test; if THIS test ends the loop the saved iterate is restored.
 * Results (z, r_his, converged) are bit-identical to residual / cycle.  Usage per iteration:
 *   residual(d) ; work = all_reduce(d, async) ; cycle_speculative() ; work.wait() ; commit(d)                        */
int smg_solve_iter_cycle_speculative(smg_hierarchy *h);
int smg_solve_iter_commit(smg_hierarchy *h, const double *d_sumsq);
int smg_solve_poll(smg_hierarchy *h, int *done, int *n_his);      /* synchronising read of the control block */
int smg_solve_end(smg_hierarchy *h, double *z, int ld_z, int memspace, double *r_his, int *n_his, int *converged);

/* The column-sharded solve as ONE call (BASELINE north_star: "C++ host code ... RCCL over xGMI only for the
 * residual-norm all-reduce"): this rank owns k_local of the k right-hand-side columns (RHS / z0 / z / known_val hold just those), the
 * hierarchy is replicated, and the library runs the reference's loop (src/min_quad_with_fixed_mg.cpp:108-125)
 *     for (iter < maxIter) { r = |RHS - A z|_F over ALL ranks' columns; push; if (r < tol) break; V-cycle }
 * itself: residual graph -> reduce(d_sumsq, 1, stream, ctx) -> cycle graph, the break test on the device from the reduced value, so
 * every rank records the same history and stops at the same iteration.  The only communication is `reduce`:
 *     int reduce(double *d_sumsq, int count, void *hip_stream, void *ctx)
 * must leave the sum over all ranks of the `count` device doubles at d_sumsq in place, ordered on hip_stream (enqueue it there --
 * ncclAllReduce(d, d, count, ncclDouble, ncclSum, comm, (hipStream_t)hip_stream) is the whole closure, examples/
 * 05_mean_curvature_flow_sharded.cpp -- or synchronise the stream and do it on the host), and return 0; any other value aborts the
 * solve with SMG_ERR_REDUCE.  It is called exactly once per loop entry, the same number of times on every rank.
 * k_local == 0 is legal (more ranks than columns): the rank contributes 0 to every reduction and follows the others' decision;
 * RHS / z0 / z may then be NULL.  Everything else (arguments, r_his / n_his / converged, memspace) as in smg_solve.
 * With world size 1 and a reduce that does nothing this IS smg_solve's loop (same graphs' kernels, same bits). */
typedef int (*smg_reduce_fn)(double *d_sumsq, int count, void *hip_stream, void *ctx);
int smg_solve_sharded(smg_hierarchy *h, const double *RHS, int ld_rhs, const double *known_val, int ld_kv, const double *z0,
                      int ld_z0, int k_local, int memspace, const smg_solve_opts *opts, smg_reduce_fn reduce, void *ctx,
                      double *z, int ld_z, double *r_his, int *n_his, int *converged);

/* ---- mg_VCycle.h pieces, host column-major blocks in the level's own (caller) numbering ------------------------ */
/* Level lv has smg_level_rows(h, lv) unknowns (after constraint elimination). */
int smg_level_rows(const smg_hierarchy *h, int lv);
int smg_vcycle(smg_hierarchy *h, const double *B, int pre, int post, int lv, double *u, int k);   /* mg_VCycle.h:22-30 */
int smg_apply_A(smg_hierarchy *h, int lv, const double *u, int k, double *Au);                    /* A()       :32-37 */
int smg_restrict(smg_hierarchy *h, int lv, const double *x, int k, double *Rx);                   /* restrict  :39-44 */
int smg_prolong(smg_hierarchy *h, int lv, const double *x, int k, double *Px);                    /* prolong   :46-51 */
int smg_relax(smg_hierarchy *h, int lv, const double *B, int k, int iters, double *u);            /* relax     :62-68 */
int smg_coarse_solve(smg_hierarchy *h, const double *B, int k, double *u);                        /* coarseSolve :70-76 */
int smg_residual_norm(smg_hierarchy *h, int lv, const double *B, const double *u, int k, double *norm);

/* ---- device-resident raw interface (internal numbering / internal row-major n x k layout) ---------------------- */
/* For benchmarks and callers that keep everything in HBM.  x, y, b: device pointers, rows in the level's
 * internal order (smg_level_get_perm), k columns interleaved.  mode: 0 y=Ax, 1 y=b-Ax, 3 y+=Ax. */
int smg_raw_spmv(smg_hierarchy *h, int lv, int mode, const double *x, const double *b, double *y, int k);
int smg_raw_relax(smg_hierarchy *h, int lv, const double *b, double *u, int k, int iters);
/* fp32 twin of smg_raw_spmv (mode 0 only): x, y are float device vectors; bytes per launch 8 nnz + 4 (n+1) + 8 n k */
int smg_raw_spmv_f32(smg_hierarchy *h, int lv, const float *x, float *y, int k);
int smg_raw_outer_iteration(smg_hierarchy *h, int n_iter);   /* residual + decide + V-cycle, n_iter times, on the
                                                                state loaded by smg_solve_begin; no host sync */
int smg_synchronize(smg_hierarchy *h);
/* diagnostic: average time (us, hipEvents on the handle's stream) of one graph-replayed V(pre,post) cycle started at level
 * lv on whatever the work vectors hold; k columns.  Used to see where a cycle's time goes level by level. */
int smg_bench_vcycle(smg_hierarchy *h, int lv, int k, int pre, int post, int reps, double *us_per_cycle);
/* diagnostic: average time (us) of `sweeps` graph-replayed Gauss-Seidel sweeps on level lv */
int smg_bench_relax(smg_hierarchy *h, int lv, int k, int sweeps, int reps, double *us_per_call);

/* ---- introspection (tests, tools) ------------------------------------------------------------------------------ */
/* which: 0 = A, 1 = P (lv >= 1), 2 = PT (lv >= 1), 3 = P_full (lv >= 1), 4 = Auk (lv == 0).
 * internal = 0: caller numbering; 1: the device numbering.  Query sizes with NULL arrays first. */
int smg_level_get_matrix(const smg_hierarchy *h, int lv, int which, int internal, int *n_rows, int *n_cols, int *nnz,
                         int *rowptr, int *col, double *val);
int smg_level_get_perm(const smg_hierarchy *h, int lv, int *perm);              /* internal -> caller, n entries */
int smg_level_get_colors(const smg_hierarchy *h, int lv, int *n_colors, int *color_ptr /* n_colors+1 or NULL */);
int smg_level_get_Adiag(const smg_hierarchy *h, int lv, double *diag);          /* mg[lv].A_diag, caller numbering */
int smg_get_unknown(const smg_hierarchy *h, int *n_unknown, int *unknown /* or NULL */);
int smg_level_sell_stats(const smg_hierarchy *h, int lv, int which, long *stored, long *padded, int *n_slices);
/* Rows of the first colour of level lv's Gauss-Seidel image whose diagonal slots the device knows (scalar hierarchies): > 0 means the
 * restriction launch of level lv - 1 can produce the first colour of this level's first sweep itself (one launch less per visit);
 * 0: not available (uncoloured / coarsest level, a row of the first colour without a stored diagonal). */
int smg_level_first_colour_rows(const smg_hierarchy *h, int lv);
/* algorithmic bytes of one y = A_lv x with k columns: 12 nnz + 4 (n+1) + 16 n k  (SURVEY.md section 8d); on a block hierarchy
 * 76 per 3 x 3 block (72 of values + 4 of block column) + 4 (n/3 + 1) + 16 n k */
long smg_level_spmv_bytes(const smg_hierarchy *h, int lv, int k);
/* algorithmic bytes of one V(pre,post) cycle incl. the outer residual evaluation, k columns -- of the cycle the handle is set to run:
 * a Chebyshev-Jacobi relax(iters) is iters + 1 passes over the level matrix, a Gauss-Seidel / Jacobi one iters passes */
long smg_vcycle_bytes(const smg_hierarchy *h, int k, int pre, int post);

/* ---- host-side self-checks (tests on boxes without a GPU; they return diagnostics only, never a solution: no CPU solve path) -------- */
/* The overlapped-tiling plan of relax(sweeps) on level lv (csrc/smg_tiled.hpp), executed on the HOST exactly as the kernel executes it
 * (tile by tile, phase by phase, tile-local numbering) on a deterministic test vector, against the plain colour-by-colour sweeps on the
 * level's matrix in the internal numbering: *max_abs_diff must be exactly 0.  Needs the host half of smg_precompute only.
 * *n_tiles = 0: the level does not qualify for tiling (too many colours, rows wider than 12 entries). */
int smg_debug_check_tiling_plan(smg_hierarchy *h, int lv, int sweeps, int tile_rows, int *n_tiles, int *max_ext_rows, double *redundancy,
                                double *max_abs_diff);
/* Test hook: builds the block Gauss-Seidel plan of level lv (smg_hierarchy_set_block_gs) on the host and executes it on the host the way the
 * kernel does, against the plain lexicographic sweep in the block order; *max_abs_diff must be 0.  Checks the plan's invariants on the way.
 * Needs no GPU (after the host half of smg_precompute).  *n_blocks = 0: the level does not qualify. */
int smg_debug_check_block_gs_plan(smg_hierarchy *h, int lv, int block_rows, int *n_blocks, int *n_colors, double *rim, double *fill, double *max_abs_diff);
/* Test hook: builds the wave Gauss-Seidel plan of level lv (smg_hierarchy_set_wave_gs; pieces_mode 0 compact pieces, 1 pieces along breadth-first level
 * sets) on the host and executes it on the host the way the kernel does, against the plain lexicographic sweep in the piece order; *max_abs_diff must be 0.
 * stats[3] as smg_level_get_wave_gs_order.  Checks the plan's invariants on the way.  Needs no GPU (after the host half of smg_precompute).
 * *n_pieces = 0: the level does not qualify (a row of more than 64 off-diagonal entries). */
int smg_debug_check_wave_gs_plan(smg_hierarchy *h, int lv, int piece_rows, int pieces_mode, int *n_pieces, int *n_colors, double *stats, double *max_abs_diff);
/* Test hook: the copies of the level values a sweep plan of level lv holds, and the maps that refresh them after a value-only smg_precompute
 * (which: 0 the overlapped tiling of relax(sweeps), sweeps 1 .. 3; 1 wave; 2 block Gauss-Seidel; sweeps is ignored for 1 and 2).  The plan is built on the
 * host from the matrix the level sweeps on -- A_lv, or its transpose where A_lv is not bit-symmetric -- exactly as the solves build it, and checked bit for
 * bit: a slot with a map holds the level value the map names, an entry slot without one +0.0 (sign bit clear), a diagonal slot without one 1.0 -- the
 * padding the refresh leaves untouched.  *n_slots: entry and diagonal slots, *n_padding: those without a map, *bad: slots that fail (must be 0).
 * against_transpose != 0: every mapped slot is compared with the MIRRORED level value (a_ji for a slot of a_ij), the comparison the map of the wrong one
 * of A_lv / A_lv^T would pass: *bad then counts the slots whose entry is not bit-symmetric.  *on_transpose: 1 when the plan was built from A_lv^T.
 * Needs no GPU (after the host half of smg_precompute; which of A_lv / A_lv^T the level sweeps on is decided with the level's images, so without a
 * GPU the hook applies that rule itself: A_lv^T wherever the two differ in any bit).  *n_slots = 0: the level has no such plan. */
int smg_debug_check_plan_value_maps(smg_hierarchy *h, int lv, int which, int sweeps, int against_transpose, int *n_slots, int *n_padding, int *bad,
                                    int *on_transpose);
/* Test hook: raises the stall flag of the sparse triangular solves on the device, as a wait that gave up would (csrc/smg_coarse_device.hip).
 * The next solve's waits then give up at once, its coarse corrections are NaN, and the next synchronising entry point returns SMG_ERR_HIP
 * and clears the flag.  Fails unless the handle holds a sparse coarse factorisation. */
int smg_debug_raise_coarse_stall(smg_hierarchy *h);
/* Test hook: the plan of the Schur-complement coarse solver built for the SPD matrix (ptr, col, val; lower triangle counts) and executed ON THE HOST
 * the way the kernels read it: x = A^-1 b.  *n_blocks = 0: no plan for this matrix (x untouched).  Needs no GPU. */
int smg_debug_schur_solve_host(int n, const int *ptr, const int *col, const double *val, const double *b, double *x, int *n_blocks, int *n_sep);
/* Test hook: the partition of the coarsest level's rows the handle's Schur-complement solver works with (csrc/smg_schur.hpp): block_of_row[r]
 * (n_coarsest entries, the coarsest level's caller numbering; NULL ok) = the interior block of row r, or -1 for a separator row.  Fails unless
 * the handle holds that solver (smg_hierarchy_coarse_solver == 2).  Needs no GPU beyond the precompute. */
int smg_debug_schur_partition(const smg_hierarchy *h, int *n_blocks, int *n_sep, int *block_of_row);
/* Sparse Cholesky of the coarse solver (csrc/smg_coarse.hpp) on an SPD matrix given in CSR (both triangles): nested-dissection order,
 * factorisation, and the relative residual |b - A x| / |b| of a host solve with the factor for a deterministic right-hand side.
 * Returns SMG_ERR_INVALID when a pivot is not positive. */
int smg_debug_check_sparse_cholesky(int n, const int *rowptr, const int *col, const double *val, long *factor_entries, int *dependency_depth,
                                    double *rel_residual);

/* Test hook: the dense generalized symmetric eigensolver of smg_eigs' Rayleigh-Ritz step, on the host.  A (symmetric) and B (symmetric
 * positive definite) are n x n column-major; out: the eigenvalues of A v = lambda B v ascending, V (n x n column-major) B-orthonormal.
 * Cholesky of B, reduction to standard form, Householder tridiagonalisation and implicit QR steps; deterministic, no LAPACK.
 * SMG_ERR_INVALID when B is not positive definite.  Needs no GPU. */
int smg_debug_dense_geneig_host(int n, const double *A, const double *B, double *evals, double *V);

/* ---- test hooks of the LOBPCG and PCG block kernels (csrc/smg_eig_device.hip, csrc/smg_krylov_device.hip) ----------------------------
 * Handle-free: each hook copies its host arrays to scratch device buffers, calls the kernels' launcher once on a private stream with a
 * control block whose `done` flag the caller picks (done = 1: every kernel must return at once and leave every output as it was), and copies
 * the outputs back.  Output arrays are in/out: their host contents are uploaded first.  Every device buffer lies between two guard regions of
 * sentinel bytes; *guard_bad (NULL ok) is the number of buffers whose guards changed, 0 when nothing was written out of place.  Blocks are
 * row-major n x m (column c of row i at i * m + c).  SMG_ERR_INVALID for a bad shape (n < 1, m outside 1..64, nb outside 1..3) or a missing
 * array; SMG_ERR_NO_DEVICE without a GPU. */
/* G (row-major a x b, a = nb_a m, b = nb_b m) = Sa^T diag(w) Sb, w == NULL: 1.  Sa, Sb: nb row-major n x m blocks back to back.
 * sym: Sb is Sa (Sb ignored, nb_b must equal nb_a), only the tiles on and above the diagonal are formed and mirrored.  *groups: the row chunks. */
int smg_debug_eig_gram(int n, int m, int nb_a, const double *Sa, int nb_b, const double *Sb, const double *w, int sym, int done, double *G,
                       int *groups, int *guard_bad);
/* With C row-major q x 2m (q = nb m):  X = S Cx, AX = AS Cx;  make_p: also P = S' Cp, AP = AS' Cp with S' the blocks 1.. of S (the rows of
 * block 0 of Cp are not read).  make_p = 0: P, AP are not handed to the launcher and may be NULL. */
int smg_debug_eig_combine(int n, int m, int nb, const double *S, const double *AS, const double *C, int make_p, int done, double *X, double *AX,
                          double *P, double *AP, int *guard_bad);
/* R = AX - diag(mass) X diag(lam); res_c = sqrt(sum_i r_ic^2 / mass_i) / |lam_c|.  f32 = 0: b0 = R, u0 = 0 (b32, u32 unused, NULL ok);
 * f32 = 1: b32 = (float) R, u32 = 0, and b0, u0 are handed to the launcher too and must come back unchanged.  *groups: the row chunks. */
int smg_debug_eig_residual(int n, int m, const double *X, const double *AX, const double *mass, const double *lam, int f32, int done, double *b0,
                           double *u0, float *b32, float *u32, double *res, int *groups, int *guard_bad);
/* One PCG launcher on n x k blocks.  v0..v3 (n x k each) are the op's operands in order, all copied back (inputs must come back unchanged):
 *   SMG_KRY_DOTS_ZR_ZQ  z, r, q      rz = z.r; beta = -alpha (z.q) / rz_prev (0 after a restart or when rz_prev == 0); clears *restart
 *   SMG_KRY_DIRECTION   z, p         p = z + beta p (p = z where beta == 0)
 *   SMG_KRY_DOTS_PQ     p, q         alpha = rz / (p.q) (0 when p.q == 0), rz_prev = rz
 *   SMG_KRY_STEP_DECIDE x, r, p, q   x += alpha p, r -= alpha q, |r|_F^2 -> the history and the break test (r < tol ends, non-finite: status -1)
 *   SMG_KRY_PRECOND_IN  r, b0, u0    b0 = r, u0 = 0
 *   SMG_KRY_WIDEN       z            z = (double) e, e: n x k floats
 * s (KS slots x k: rz, rz_prev, alpha, beta; ops up to STEP_DECIDE) and *restart (NULL: 0) are in/out.  The control block starts with
 * sumsq = -1, a one-entry history holding -1, n_his = status = 0; out: ctrl_d = {sumsq, r_his[0]}, ctrl_i = {n_his, done, status} (NULL ok).
 * *groups: the row chunks of the reductions. */
enum { SMG_KRY_DOTS_ZR_ZQ = 0, SMG_KRY_DIRECTION = 1, SMG_KRY_DOTS_PQ = 2, SMG_KRY_STEP_DECIDE = 3, SMG_KRY_PRECOND_IN = 4, SMG_KRY_WIDEN = 5 };
int smg_debug_krylov(int op, int n, int k, double *v0, double *v1, double *v2, double *v3, float *e, double *s, int *restart, double tol, int done,
                     double *ctrl_d, int *ctrl_i, int *groups, int *guard_bad);
/* ---- test hooks of the fp32 V-cycle (precision = 1: enqueue_vcycle_t<float>, csrc/smg_cycle.cpp), piece by piece ----------------------------
 * Like the fp64 pieces (smg_apply_A ... smg_vcycle) these take host column-major blocks in the caller's numbering of the level (n_lv x k floats,
 * leading dimension n_lv), refuse a handle in a split-phase solve, a union handle and a sparse coarse factorisation, and use the handle's
 * current smoother (smg_hierarchy_set_smoother).  Each op launches what the fp32 cycle launches for that piece, on the handle's own fp32
 * vectors (b32, u32, r32, t32, d32 of the levels) and with the handle's control block, whose `done` flag the caller picks: with done != 0
 * every launch must return without writing.  `out` is in/out: its host contents are uploaded to every buffer the op writes and read back
 * afterwards.  *inputs_changed (NULL ok): bit 0 is set when a buffer the op only reads no longer holds what was uploaded; bit 2 when, with
 * done != 0, any fp32 vector of the cycle -- b32, u32, r32, the second iterate t32 and the update vector d32 of EVERY level, the Schur solver's
 * separator vectors -- differs after the launches from what it held after the uploads.
 *   SMG_F32_A            in0 = x (level lv)                  out = A x
 *   SMG_F32_RESID        in0 = b, in1 = x                    out = b - A x
 *   SMG_F32_RESTRICT     in0 = r (level lv)                  out = [PT r | uc], two n_{lv+1} x k blocks back to back: the restriction launch without
 *                                                            a fused first launch writes the coarse right-hand side and zeroes the coarse iterate
 *   SMG_F32_PROLONG_ADD  in0 = uc (level lv + 1)             out (level lv) += P uc
 *   SMG_F32_RELAX        in0 = b                             out = relax(pre) of out: `pre` sweeps of Gauss-Seidel (one launch per colour) or damped
 *                                                            Jacobi, or ONE Chebyshev polynomial of degree pre + 1 (pre = 0: nothing)
 *   SMG_F32_COARSE       in0 = b (coarsest level, lv unused) out += A^-1 b, dense inverse or Schur complement, as the handle chose
 *   SMG_F32_VCYCLE       in0 = b                             out = V(pre, post) from level lv: the launch sequence of the mixed-precision solve,
 *                                                            with its fused first launches (SMG_FUSE_FIRST) and its buffer ping-pong
 * Block (3-DOF) hierarchies: the same, on rows 3 v + d. */
enum { SMG_F32_A = 0, SMG_F32_RESID = 1, SMG_F32_RESTRICT = 2, SMG_F32_PROLONG_ADD = 3, SMG_F32_RELAX = 4, SMG_F32_COARSE = 5, SMG_F32_VCYCLE = 6 };
int smg_debug_cycle_f32(smg_hierarchy *h, int op, int lv, int k, int pre, int post, int done, const float *in0, const float *in1, float *out,
                        int *inputs_changed);
/* The two converters between the fp64 outer loop and the fp32 cycle, on level 0's vectors (n_0 x k blocks as above):
 *   SMG_F32_RESIDUAL_TO_F32  in64 = r            out_b32 = (float) r, out_u32 = 0        (in32, out64 unused)
 *   SMG_F32_ADD_CORRECTION   in32 = e            out64 (in/out) = z + (double) e          (in64, out_b32, out_u32 unused)
 * *inputs_changed: bit 0 as above; bit 1 is set when the launch wrote behind the n_0 x k block (the room a handle that has served more
 * columns keeps there is filled with sentinel bytes for the launch). */
enum { SMG_F32_RESIDUAL_TO_F32 = 0, SMG_F32_ADD_CORRECTION = 1 };
int smg_debug_convert_f32(smg_hierarchy *h, int op, int k, int done, const double *in64, const float *in32, double *out64, float *out_b32,
                          float *out_u32, int *inputs_changed);
/* Test hook, read-only: the side of the size gate of the multi-column SELL launches (csrc/smg_device.hip: launch_wide_one) a launch of n_slices
 * slices takes for a block of kw in {8, 16, 32} columns in THIS process: 1 = one row per lane with the whole row in flight (k_sell_wide<.., R = 1,
 * U = 8 / 16 / 32>), 0 = the streaming kernel with two rows per lane (R = 2, U = 8).  n_slices * kw <= SMG_WIDE_LAT_MAX (default 16384, read once
 * per process) selects the former.  Blocks of 64 columns have one variant and do not consult the gate.  Needs no GPU. */
int smg_debug_wide_latency_variant(int n_slices, int kw);
/* Test hooks, read-only, no device work: which instantiations of the wave Gauss-Seidel kernel k_wgs<NBMAX, KB, RIMI> (csrc/smg_wgs_device.hip) run in
 * THIS process.  They answer through the functions launch_wgs itself calls, whose knobs (SMG_WGS_KB2_MAX_PIECES, default 1600; SMG_WGS_KB_SMALL,
 * default 1; SMG_WGS_KB_BIG, default 4) are read once per process.
 * smg_debug_wgs_launches: the launches one piece colour of a sweep takes for k columns on a plan of n_pieces pieces whose widest row needs nb_max
 *   batches of 8 entry slots and whose rim pitch is rim_pitch: *nbmax = 3 / 5 / 8 (nb_max <= 3, <= 5, <= 8), *rimi = 2 / 4 / 7 (rim_pitch 128 / 256 /
 *   448), launches[2 i], launches[2 i + 1] = (KB columns per lane, groups in the grid's second dimension) of launch i for i < min(*n_launches, cap).
 *   The launches cover columns 0 .. k - 1 in order.  SMG_ERR_INVALID for a plan the kernel has no variant for.  Needs no GPU.
 * smg_debug_wgs_level_plan: n_pieces, nb_max and rim_pitch of the plan of level lv.  from_host 0: the plan relax() sweeps with for k columns in the
 *   handle's present state; nothing is built -- *n_pieces = 0 where the level sweeps another way (colour launches, the one-launch relax) or no sweep
 *   has asked for the plan yet.  from_host 1: the plan as the first sweep would build it, built on the host and dropped (no GPU needed after the
 *   host half of smg_precompute); *n_pieces = 0: the level does not qualify (a row of more than 64 off-diagonal entries, a rim above 448 rows). */
int smg_debug_wgs_launches(int n_pieces, int nb_max, int rim_pitch, int k, int *nbmax, int *rimi, int *launches, int cap, int *n_launches);
int smg_debug_wgs_level_plan(smg_hierarchy *h, int lv, int k, int from_host, int *n_pieces, int *nb_max, int *rim_pitch);
/* Test hook, read-only, no device work: the launches that y = A x (mode 0) or y = b - A x (mode 1) with 1 <= k <= 4 fp64 columns -- one narrow group of
 * launch_sell_mode (csrc/smg_device.hip) -- take on the device image `which` (0 A, 1 P, 2 PT) of level lv in THIS process, through the function the
 * launcher itself calls (SMG_DEEP, SMG_DEEP_MIN_W: read once per process).  *w_max: panel columns of the image's widest slice;
 * launches[2 i] = columns per lane, launches[2 i + 1] = 3 / 5 / 8, the row-width class of k_sell_deep (w_max <= 24: at most 3 columns per lane,
 * <= 40: 2, <= 64: 1 -- four columns go 3 + 1, 2 + 2 or 1 + 1 + 1 + 1), or 0: k_sell.  Needs the device half of smg_precompute. */
int smg_debug_deep_launches(const smg_hierarchy *h, int lv, int which, int mode, int k, int *w_max, int *launches, int cap, int *n_launches);
/* Test hook, read-only, no device work: *wpb = the waves per workgroup (2, 4 or 8) of a one-column Gauss-Seidel colour launch of n_slices slices on
 * the image level lv sweeps on, in THIS process, through the function launch_narrow itself branches on: SMG_GS_WPB (default 4) = 2 / 8 selects
 * k_sell<SELL_GS, 1, T, 7, 2 / 8> where the image has fixed-pitch panels of lower width 7, the launch is not confined to one XCD (SMG_ONE_XCD_MAX) and
 * does not request the whole pitch ahead (SMG_PITCH_SPEC_MAX); 4 otherwise.  *stride, *w_lo (optional): the image's panel pitch (0: compact panels)
 * and lower width.  Needs the device half of smg_precompute. */
int smg_debug_gs_colour_wpb(const smg_hierarchy *h, int lv, int n_slices, int *wpb, int *stride, int *w_lo);
/* One launcher of the heat-method geodesics (csrc/smg_geodesics_device.hip), handle-free and guarded like the hooks above.  Blocks are
 * column-major n x k; `in` has leading dimension n, `out` has ld_out >= n and is in/out.  Source lists: src_ptr[0] = 0, k non-empty sets.
 *   SMG_GEO_BASIS       in = V (n x 3 row-major), F (nF x 3) -> W[9f + 3i + d] = ((N x e_i) / (2A))_d, Af[f] = A   (out unused)
 *   SMG_GEO_SCATTER     src_ptr, src -> out = the indicator block (1 at column c's sources, 0 elsewhere)
 *   SMG_GEO_DIVERGENCE  F, W, Af, m_ptr[n + 1], m_idx (the corner lists t = 3f + j of each vertex), in = u -> out = -div X, X = -grad u / |grad u|
 *   SMG_GEO_SHIFT       src_ptr, src, in = phi -> out = phi - (the mean of phi over column c's sources, list order)
 * SMG_ERR_INVALID for an unknown op, a bad shape, an index out of range or an empty source set; SMG_ERR_NO_DEVICE without a GPU. */
enum { SMG_GEO_BASIS = 0, SMG_GEO_SCATTER = 1, SMG_GEO_DIVERGENCE = 2, SMG_GEO_SHIFT = 3 };
int smg_debug_geodesics(int op, int n, int nF, int k, const int *F, const int *m_ptr, const int *m_idx, const int *src_ptr, const int *src,
                        const double *in, double *W, double *Af, double *out, int ld_out, int *guard_bad);
/* One launcher of the ARAP local step (csrc/smg_arap_device.hip), handle-free and guarded like the hooks above.  rowptr[n + 1], col, w: a CSR
 * matrix with n rows and columns (rowptr[0] = 0; diagonal entries are skipped, N(i) = the other entries of row i in stored order); P0, P:
 * rest and current positions, n x 3 row-major; R_in: n rotations, 9 doubles each, row-major.  out is in/out.
 *   SMG_ARAP_COVARIANCE     P0, P        -> out[9i + 3a + c] = sum_j (w_ij e_ij,a) e'_ij,c, e_ij = p_i - p_j
 *   SMG_ARAP_ROTATIONS      P0, P        -> out[9i ..] = the rotation R_i that maximises tr(R_i S_i)
 *   SMG_ARAP_RHS            P0, R_in     -> out (n x 3 column-major) = b, b_i = sum_j (w_ij / 2) (R_i + R_j) e_ij     (P may be NULL)
 *   SMG_ARAP_VERTEX_ENERGY  P0, P, R_in  -> out[i] = sum_j w_ij |e'_ij - R_i e_ij|^2
 *   SMG_ARAP_ENERGY         P0, P, R_in  -> out[0] = the sum of those terms (fixed row chunks, fixed-order finalize)
 * SMG_ERR_INVALID for an unknown op, a missing operand or a bad CSR structure; SMG_ERR_NO_DEVICE without a GPU. */
enum { SMG_ARAP_COVARIANCE = 0, SMG_ARAP_ROTATIONS = 1, SMG_ARAP_RHS = 2, SMG_ARAP_VERTEX_ENERGY = 3, SMG_ARAP_ENERGY = 4 };
int smg_debug_arap(int op, int n, const int *rowptr, const int *col, const double *w, const double *P0, const double *P, const double *R_in,
                   double *out, int *guard_hits);
/* The fixed-order reduction under every energy, stopping test and CFL rate (csrc/smg_fixed_sum_device.hip), handle-free and guarded like the
 * hooks above, at a length of the caller's choosing: *out = the sum (SMG_FIXED_SUM: launch_fixed_sum) or the maximum (SMG_FIXED_MAX:
 * launch_fixed_max; a NaN loses against a number, n NaNs give -inf) of term[0 .. n).  The chunk scratch holds exactly the launched chunk count
 * of doubles and the result one double, each between guards; *groups (NULL ok): the chunk count that was launched.
 * SMG_ERR_INVALID for an unknown op, n <= 0 or a NULL term / out; SMG_ERR_NO_DEVICE without a GPU. */
enum { SMG_FIXED_SUM = 0, SMG_FIXED_MAX = 1 };
int smg_debug_fixed_reduce(int op, int n, const double *term, double *out, int *groups, int *guard_bad);

/* One launcher of the membrane step (csrc/smg_membrane_device.hip), handle-free and guarded like the hooks above.  V0: the rest pose, P: a pose,
 * both nV x 3 row-major; per-face arrays are planes (entry e of face f at [e nF + f]); in / out are concatenations in the order given:
 *   SMG_MEM_REST        V0                 -> out = rest constants (5 planes): (abar^-1)00, 01, 11, det abar, coeff
 *   SMG_MEM_FACES_RAW   V0, P              -> out = W (nF), G (9 planes), the upper triangle of the UNFIXED H_f (45 planes)
 *   SMG_MEM_FACES       V0, P              -> the same with the eigenvalue fix
 *   SMG_MEM_ENERGY      V0, P              -> out = W (nF) by the energy-only kernel of the line search
 *   SMG_MEM_PRESSURE    P                  -> out = e1 x e2 (3 planes), corner shares of the Voronoi mass (3 planes), m (nV), fext (3 nV)
 *   SMG_MEM_MATRIX      in = H (45 planes), mass0 (nV)                                   -> out = the values of H = M + dt^2 K (9 n_blocks)
 *   SMG_MEM_GRADIENT    in = G (9 planes), mass0 (nV), qdot, qdot0, fext (3 nV each)        -> out = g (3 nV), b (3 nV)
 *   SMG_MEM_OBJECTIVE   V0, P = pos0, in = mass0 (nV), qdot, dx, qdot0, fext (3 nV each), step (1)
 *                                          -> out = t (3 nV), pos0 + dt t (3 nV), the terms (nF faces, then nV vertices), f (1) */
enum { SMG_MEM_REST = 0, SMG_MEM_FACES_RAW = 1, SMG_MEM_FACES = 2, SMG_MEM_ENERGY = 3, SMG_MEM_PRESSURE = 4, SMG_MEM_MATRIX = 5,
       SMG_MEM_GRADIENT = 6, SMG_MEM_OBJECTIVE = 7 };
int smg_debug_membrane(int op, int nV, int nF, const int *F, const double *V0, const double *P, const double *in, const smg_membrane_params *p,
                       double *out, int *guard_hits);
/* The same ops on the kernels of a material (smg_membrane_set_material: 0, 1, 2; another value: SMG_ERR_INVALID). */
int smg_debug_membrane_material(int material, int op, int nV, int nF, const int *F, const double *V0, const double *P, const double *in,
                                const smg_membrane_params *p, double *out, int *guard_hits);

/* One launcher of the disk parameterization (csrc/smg_param_device.hip), handle-free and guarded like the hooks above.  F: nF x 3, V0: nV x 3
 * row-major, UV: nV x 2 column-major (leading dimension nV), R_in: the rotations as 2 planes (cos, sin); per-face results are planes (entry e
 * of face f at [e nF + f]).  out is in/out.
 *   SMG_PARAM_REST         V0               -> out = the rest constants (6 planes): x1.x, x2.x, x2.y, c0, c1, c2
 *   SMG_PARAM_COVARIANCE   V0, UV           -> out = S_f (4 planes): S00, S01, S10, S11
 *   SMG_PARAM_ROTATIONS    V0, UV           -> out = R_f (2 planes): cos, sin
 *   SMG_PARAM_RHS          V0, R_in         -> out (nV x 2 column-major) = the right-hand side of the global step
 *   SMG_PARAM_FACE_ENERGY  V0, UV, R_in     -> out[f] = (1/2) sum_i c_i |(u_i - u_{i+1}) - R_f (x_i - x_{i+1})|^2
 *   SMG_PARAM_ENERGY       V0, UV, R_in     -> out[0] = the sum of those terms (fixed row chunks, fixed-order finalize)
 *   SMG_PARAM_DISTORTION   V0, UV           -> out = det J, sigma1, sigma2 (3 planes)
 * SMG_ERR_INVALID for an unknown op, a missing operand or a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
enum { SMG_PARAM_REST = 0, SMG_PARAM_COVARIANCE = 1, SMG_PARAM_ROTATIONS = 2, SMG_PARAM_RHS = 3, SMG_PARAM_FACE_ENERGY = 4, SMG_PARAM_ENERGY = 5,
       SMG_PARAM_DISTORTION = 6 };
int smg_debug_param(int op, int nV, int nF, const int *F, const double *V0, const double *UV, const double *R_in, double *out, int *guard_hits);

/* One launcher of the projective-dynamics step (csrc/smg_pd_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V0 (the rest
 * pose) and P (a pose): nV x 3 xyz rows; p: dt, density, stiffness, the band, pressure and gravity of the op; per-face results are planes (entry e
 * of face f at [e nF + f]); column-major blocks are nV x 3 with leading dimension nV; in / out are concatenations in the order given.
 *   SMG_PD_REST       V0              -> out = the rest constants (4 planes): a, b, c, A_f
 *   SMG_PD_FACES      V0, P           -> out = Fg (6 planes), sigma (2), T (6), the energy terms (1), the corner shares (9): k_pd_faces<1>
 *   SMG_PD_FACES_STEP V0, P           -> out = the energy terms (1), the corner shares (9): k_pd_faces<0>, the pose read as a column-major block
 *   SMG_PD_MASS       V0              -> out = m0 (nV), the Voronoi mass of the rest pose as the object computes it
 *   SMG_PD_PREDICT    V0, P = x, in = vel (3 nV xyz rows) -> out = fext (3 nV xyz rows), S (column-major)
 *   SMG_PD_VERTICES   in = the corner shares (9 planes), m0 (nV), S, Q (column-major each)
 *                                     -> out = B (column-major), the inertia terms (nV), |B_v|^2 (nV)
 *   SMG_PD_ENERGY     in = terms (nF + nV) -> out[0] = their sum (fixed row chunks, fixed-order finalize)
 *   SMG_PD_FINISH     P = x, in = Q (column-major) -> out = vel = (Q - x) / dt (3 nV xyz rows), the new x (3 nV xyz rows)
 *   SMG_PD_STRAIN     V0, P           -> out = the statistics' terms (5 planes): sigma1, -sigma2, outside the band, A_f |F - T|_F^2, A_f
 * SMG_ERR_INVALID for an unknown op, a missing operand or a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
enum { SMG_PD_REST = 0, SMG_PD_FACES = 1, SMG_PD_FACES_STEP = 2, SMG_PD_MASS = 3, SMG_PD_PREDICT = 4, SMG_PD_VERTICES = 5, SMG_PD_ENERGY = 6,
       SMG_PD_FINISH = 7, SMG_PD_STRAIN = 8 };
int smg_debug_pd(int op, int nV, int nF, const int *F, const double *V0, const double *P, const double *in, const smg_pd_params *p, double *out,
                 int *guard_hits);

/* One launcher of the denoiser (csrc/smg_denoise_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V0 (the input mesh) and P
 * (a pose): nV x 3 xyz rows; p: sigma_s, sigma_r, normal_iters and fidelity of the op; per-face arrays are planes (entry e of face f at
 * [e nF + f]); column-major blocks are nV x 3 with leading dimension nV; in / out are concatenations in the order given.  N(f) is built from F.
 *   SMG_DN_REST     V0                       -> out = the rest constants (10 planes): n (3), A, c (3), w (3)
 *   SMG_DN_SPACING  V0                       -> out[f] = the sum over N(f), list order, of |c_f - c_g|
 *   SMG_DN_FILTER   V0, in = normals (3 planes) -> out = the normals after normal_iters iterations (3 planes); sigma_s must be > 0 here
 *   SMG_DN_PROJECT  V0, P, in = m (3 planes) -> out = the energy terms (1), the corner shares (9); the pose read as a column-major block
 *   SMG_DN_RHS      V0, in = the corner shares (9 planes), X (column-major)
 *                                            -> out = B (column-major), the fidelity terms (nV), |B_v|^2 (nV), the mass M (nV)
 *   SMG_DN_ENERGY   in = terms (nF + nV)     -> out[0] = their sum (fixed row chunks, fixed-order finalize)
 * SMG_ERR_INVALID for an unknown op, a missing operand, a face index out of range or a filter without sigma_s > 0; SMG_ERR_NO_DEVICE without a
 * GPU. */
int smg_debug_denoise(int op, int nV, int nF, const int *F, const double *V0, const double *P, const double *in, const smg_denoise_params *p,
                      double *out, int *guard_hits);

/* One launcher of the stylizer (csrc/smg_stylize_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; rowptr[nV + 1], col, w: a
 * CSR with the cotangent matrix's pattern (diagonal entries are skipped); V0 (the rest mesh) and P (a pose): nV x 3 xyz rows; lambda: nV values
 * or NULL = p->lambda; Q: 9 doubles or NULL = the identity; targets: nV x 3 xyz rows; state_in: 7 planes of nV (z, u, rho) or NULL = the start
 * state z = u = 0, rho = p->rho0; R_in: 9 doubles per vertex.  n_i and a_i are computed from F and V0 by k_stylize_normals first.
 *   SMG_STY_NORMALS        V0                 -> out = n (nV x 3 xyz rows), a (nV)
 *   SMG_STY_ADMM_ONE       V0, P, [state_in]  -> exactly one ADMM iteration: the layout of SMG_STY_LOCAL, iters all 1
 *   SMG_STY_LOCAL          V0, P, [state_in]  -> out = R (9 nV), the energy terms (nV), the state (7 planes); iters[nV] = the iterations used
 *   SMG_STY_LOCAL_TARGETS  V0, P, targets     -> out = R (9 nV), the energy terms (nV); iters all 0
 *   SMG_STY_ENERGY         V0, P, R_in, [targets: the normal-driven term] -> out = the energy terms (nV), then their sum (fixed row chunks,
 *                                                fixed-order finalize)
 * SMG_ERR_INVALID for an unknown op, a missing operand, bad parameters, a face index out of range or a malformed CSR; SMG_ERR_NO_DEVICE without
 * a GPU. */
int smg_debug_stylize(int op, int nV, int nF, const int *F, const int *rowptr, const int *col, const double *w, const double *V0, const double *P,
                      const double *lambda, const double *Q, const double *targets, const double *state_in, const double *R_in,
                      const smg_stylize_params *p, double *out, int *iters, int *guard_hits);

/* One launcher of the morpher (csrc/smg_morph_device.hip), handle-free and guarded like the hooks above.  (V0, F): a rest mesh, nV x 3 xyz rows
 * and nF x 3; k sets; every array is host.  The rest basis, normals and areas are computed from F and V0 by k_morph_basis first where an op reads
 * them.
 *   SMG_MORPH_FACE_GRADIENT  X = k poses (k x nV x 3)         -> out = J, k sets of nF x 9 (the rest basis formed inside the kernel)
 *   SMG_MORPH_FACE_POLAR     X = one pose                     -> out = R (9 nF), omega (3 nF), S (6 nF)
 *   SMG_MORPH_RHS_GRADIENT   in = J (k sets of nF x 9)        -> out = B (nV x 3k column-major), |b_v|^2 (k planes of nV)
 *   SMG_MORPH_RHS_INTERP     in = omega (3 nF), S (6 nF); t[k] -> out = B, |b_v|^2 as above
 *   SMG_MORPH_PINS           pins[n_pins]; X = one pose with t[k], or NULL = the rest pose
 *                                                             -> out = the pins' default positions (n_pins x 3k column-major), then the default
 *                                                                start (nV x 3k column-major) with its pinned rows set from them
 * SMG_ERR_INVALID for an unknown op, a missing operand, k < 1, a non-finite t, a face index or a pin out of range; SMG_ERR_NO_DEVICE without
 * a GPU. */
int smg_debug_morph(int op, int nV, int nF, int k, const int *F, const double *V0, const double *X, const double *t, const double *in,
                    const int *pins, int n_pins, double *out, int *guard_hits);

/* One launcher of the flow (csrc/smg_flow_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; U and V0: nV x 3 column-major
 * blocks with leading dimension nV; every array is host.
 *   SMG_FLOW_SYSTEM      U; (rowptr, col, L0): a CSR with one stored diagonal entry per row; delta
 *                        -> out = the barycentric masses of U (nV), mass U (nV x 3 column-major), (-delta) L0 with the mass added on the diagonal
 *   SMG_FLOW_NORMALIZE   U -> out = normalize_unit_area of U (nV x 3 column-major)
 *   SMG_FLOW_SPHERICITY  U -> out = 7 doubles: the sphericity, sum a, sum a U (3), sum a r, sum a (r - rbar)^2
 *   SMG_FLOW_SPHERE      U, V0 = the rest mesh -> out = S (nV x 3 column-major), sigma (2 planes of nF), the terms (4 planes of nF:
 *                        A sigma1 / sigma2, A, sigma1 / sigma2, flipped), the 4 stats of smg_flow_sphere
 * SMG_ERR_INVALID for an unknown op, a missing operand, a face index out of range, and for the system a delta that is not finite or <= 0 or a
 * malformed CSR; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_flow(int op, int nV, int nF, const int *F, const double *U, const double *V0, const int *rowptr, const int *col, const double *L0,
                   double delta, double *out, int *guard_hits);

/* One launcher of the Hodge decomposition (csrc/smg_hodge_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V: nV x 3
 * row-major; X: k fields of nF x 3 row-major; u, v: nV x k column-major with leading dimension nV; every array is host.  k_hodge_geometry runs
 * first on buffers of its own.
 *   SMG_HODGE_RHS    V, X -> out = b (nV x k column-major), c (nV x k column-major), their squares (2 planes of k nV: b^2 then c^2)
 *   SMG_HODGE_PARTS  V, X, u, v -> out = the parts (k sets of nF x 9: G, R, H), the terms (4 k planes of nF: plane 4 c + e = A_f |.|^2 of Xt, G, R,
 *                    H of field c), the 4 k energies
 *   SMG_HODGE_FIELD  V, u, v -> out = X (k fields of nF x 3)
 * SMG_ERR_INVALID for an unknown op, a missing operand, k < 1, a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_hodge(int op, int nV, int nF, int k, const int *F, const double *V, const double *X, const double *u, const double *v, double *out,
                    int *guard_hits);

/* One launcher of the conformal metric (csrc/smg_conformal_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; l0: nF x 3, the
 * rest length of the edge opposite every corner; area2: nF, twice the rest area of every face (the cross product's norm); u, d, s, Theta: nV; fixed: n_fixed vertex indices (may be empty); every array is host.
 *   SMG_CONFORMAL_SCALE  u; d (NULL ok) and t: the trial u + t d -> out = s = exp(-(u + t d) / 2) (nV), then u + t d (nV)
 *   SMG_CONFORMAL_FACES  l0, area2, s -> out = the angles (nF x 3), the half cotangents (nF x 3), the broken flags (nF, 1.0 / 0.0), l~ (nF x 3)
 *   SMG_CONFORMAL_ROWS   l0, area2, s, Theta, fixed -> out = the angle sums (nV), g (nV), g^2 (nV), |g| (nV), then sum g^2, max |g| and the broken count,
 *                        then the values of -L~ in smg_mesh_cotmatrix's CSR order (its nnz doubles); k_conformal_faces runs first on buffers of its own
 * SMG_ERR_INVALID for an unknown op, a missing operand, a face index out of range, a non-finite t, a fixed vertex out of range or listed twice;
 * SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_conformal(int op, int nV, int nF, const int *F, const double *l0, const double *area2, const double *u, const double *d, double t,
                        const double *s, const double *Theta, const int *fixed, int n_fixed, double *out, int *guard_hits);

/* One launcher of the earth mover's distance (csrc/smg_emd_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V: nV x 3
 * row-major; b, phi: nV x k column-major with leading dimension nV; rho: k; every array is host.  k_emd_geometry runs first where an op reads W2.
 *   SMG_EMD_GEOMETRY  V -> out = W2 (nF x 6), A (nF), their fixed-order sum (1)
 *   SMG_EMD_RHS       V, b, state = ZU (k sets of nF x 4) -> out = r (nV x k column-major)
 *   SMG_EMD_UPDATE    V, phi, state = ZU, rho, alpha -> out = ZU (k sets of nF x 4), J (k sets of nF x 2), the planes A |J| and rho^2 |grad phi|^2
 *                     (k planes of nF each), their fixed-order sums (k) and maxima (k)
 *   SMG_EMD_DUAL      b, phi, rho, state = gmax^2 (k) -> out = the potential (nV x k column-major), the terms b potential (k planes of nV), their sums (k)
 *   SMG_EMD_FLOW      V, state = J (k sets of nF x 2) -> out = J in 3-D (k sets of nF x 3)
 *   SMG_EMD_RESIDUAL  V, b, state = J -> out = d = the weak divergence of J minus b (nV x k column-major), its squares with vertex 0's zero (k planes
 *                     of nV), their sums (k)
 * SMG_ERR_INVALID for an unknown op, nV < 1, nF < 1, a missing operand, k < 1, a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_emd(int op, int nV, int nF, int k, const int *F, const double *V, const double *b, const double *phi, const double *state,
                  const double *rho, double alpha, double *out, int *guard_hits);

/* One launcher of the surface fluid (csrc/smg_fluid_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V: nV x 3 row-major;
 * w, psi, wn: nV x k column-major with leading dimension nV; dt: k; every array is host.  k_hodge_geometry and k_fluid_mass run first; the known
 * rows are the boundary vertices, or vertex 0 on a closed mesh, and wbar is 0 on a mesh with boundary.
 *   SMG_FLUID_RHS       V, w -> out = m (nV), its sum (1), the terms m w (k planes of nV), their sums (k), r (nV x k column-major), its squares
 *                       with the known rows' zero (k planes of nV), their one sum (1)
 *   SMG_FLUID_ADVECT    V, psi, w, wn, a, b, dt, theta -> out = the stage's output (nV x k column-major), the rates (k planes of nV), the terms
 *                       m out (k planes of nV), the rates' maxima (k), the terms' sums (k); rates_only != 0: V, psi -> the rates, their maxima
 *   SMG_FLUID_VELOCITY  V, psi -> out = U (k sets of nF x 3), the terms (1/2) A |grad psi|^2 (k planes of nF), their sums (k)
 *   SMG_FLUID_DIAG      V, w -> out = the terms m w and (1/2) m w^2 (k planes of nV each), their sums (k each)
 *   SMG_FLUID_DT        w = the maxima of three stages (3 x k row-major), psi = the times (k), a = cfl -> out = dt (k) of the first row, the
 *                       three-stage step's cfl (k), the times after it (k)
 * SMG_ERR_INVALID for an unknown op, nV < 1, nF < 1, a missing operand, k < 1, theta outside [0, 1], a face index out of range;
 * SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_fluid(int op, int nV, int nF, int k, const int *F, const double *V, const double *w, const double *psi, const double *wn, double a,
                    double b, const double *dt, double theta, int rates_only, double *out, int *guard_hits);
/* The time of one launcher of the surface fluid alone, for tools/fluid_time.py: SMG_FLUID_RHS, _ADVECT (rates_only as above), _VELOCITY or _DIAG on
 * device blocks of zeros of k columns over the mesh (F, V: host), launched `reps` times back to back on one stream between two events after one
 * launch that is not timed; *ms = the mean time of a launch in milliseconds.  SMG_ERR_INVALID for another op, nV < 1, nF < 1, a missing array,
 * k < 1, reps < 1, a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_fluid_time(int op, int nV, int nF, int k, const int *F, const double *V, int rates_only, int reps, double *ms);

/* One launcher of the reaction-diffusion object (csrc/smg_rd_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V: nV x 3
 * row-major; u, v, un, vn: nV x k column-major with leading dimension nV; coeff: k x 20 row-major; every array is host.  k_hodge_geometry and
 * k_fluid_mass run first.
 *   SMG_RD_REACT  V, u, v, coeff, dt, substeps -> out = the right-hand sides m u* then m v* (nV x 2k column-major), their squares (2k planes of
 *                 nV), v* (nV x k column-major), the sums of the squares of m u* and of m v* (2)
 *   SMG_RD_CLOSE  V, u, v (the step's start), un, vn (its end) -> out = the terms m un then m vn (2k planes of nV), the changes (k planes of nV),
 *                 the terms' sums (2k), the changes' maxima (k)
 * SMG_ERR_INVALID for an unknown op, nV < 1, nF < 1, a missing operand, k < 1, substeps < 1, dt not finite and > 0, a non-finite coefficient, a
 * face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_rd(int op, int nV, int nF, int k, const int *F, const double *V, const double *u, const double *v, const double *coeff, double dt,
                 int substeps, const double *un, const double *vn, double *out, int *guard_hits);
/* The time of one launcher of the reaction-diffusion object alone, for tools/rd_time.py: SMG_RD_REACT (with `substeps` sub-steps) or SMG_RD_CLOSE
 * on device blocks of zeros of k columns over the mesh (F, V: host), launched `reps` times back to back on one stream between two events after
 * one launch that is not timed; *ms = the mean time of a launch in milliseconds.  SMG_ERR_INVALID for another op, nV < 1, nF < 1, a missing
 * array, k < 1, substeps < 1, reps < 1, a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_rd_time(int op, int nV, int nF, int k, const int *F, const double *V, int substeps, int reps, double *ms);

/* One launcher of the wave object (csrc/smg_wave_device.hip), handle-free and guarded like the hooks above.  F: nF x 3; V: nV x 3 row-major;
 * speed, sigma: nV or NULL (1 and 0 everywhere); u, v, w: nV x k column-major with leading dimension nV; idx: n_idx vertices; sig0, sig1: n_idx x k
 * row-major; every array is host.  k_hodge_geometry and k_fluid_mass run first; mt = m / speed^2 and s2 = 2.0 + sigma dt are formed on the host
 * from the device's masses; clamped = 1: the boundary vertices are the known rows.  a = 0.25 dt dt, q2 = 2.0 / dt.
 *   SMG_WAVE_RHS      u, v -> out = b (nV x k column-major), its squares (k planes of nV), the warm start (nV x k), the squares' sum (1)
 *   SMG_WAVE_SOURCES  u, v, idx, sig0, sig1 -> k_wave_rhs, then k_wave_sources: out as for SMG_WAVE_RHS
 *   SMG_WAVE_ADVANCE  u, v, w -> out = u', v' (nV x k each) and the kinetic terms (k planes of nV) of a launch without the next right-hand side;
 *                     the same three of a launch with it, then its b, squares and warm start (nV x k each); the kinetic sums (k), the potential
 *                     sums (k: k_fluid_velocity's terms of u'), the squares' sum (1)
 *   SMG_WAVE_RECORD   u, idx -> out = u at the vertices idx (n_idx x k row-major); F and V are only checked
 * SMG_ERR_INVALID for an unknown op, nV < 1, nF < 1, a missing operand, k < 1, dt not finite and > 0, clamped not 0 or 1, a speed not finite and
 * > 0, a sigma not finite and >= 0, a face index out of range, n_idx < 1, a list index out of range, a source listed twice; SMG_ERR_NO_DEVICE
 * without a GPU. */
int smg_debug_wave(int op, int nV, int nF, int k, const int *F, const double *V, const double *speed, const double *sigma, int clamped, double dt,
                   const double *u, const double *v, const double *w, const int *idx, int n_idx, const double *sig0, const double *sig1, double *out,
                   int *guard_hits);
/* One launcher of the wave object's adjoint pass (csrc/smg_wave_adjoint_device.hip), handle-free and guarded like the hooks above.  F, V, speed, sigma,
 * clamped, dt: as smg_debug_wave (mt, s2 and the factor plane are formed on the host from the device's masses; q2 = 2.0 / dt, a = 0.25 dt dt).
 * Vertex blocks are nV x k column-major with leading dimension nV; a trace row is n_idx slots x k row-major; every array is host.
 *   SMG_WAVE_ADJ_KEEP      x0 = u, x1 = v, x2 = u' -> out = e (nV x k)
 *   SMG_WAVE_ADJ_RESIDUAL  x0 = traces, x1 = observed or NULL (n_rows x n_idx x k each) -> out = rho (the same layout), its squares (k planes of
 *                          n_rows x n_idx), the k fixed-order sums of the planes; F and V are only checked
 *   SMG_WAVE_ADJ_INJECT    x0 = p, x1 = rho (one row: n_idx x k), idx = the receivers (a vertex may repeat) -> out = p + R' rho (nV x k)
 *   SMG_WAVE_ADJ_RHS       x0 = p, x1 = q -> out = g (nV x k), its squares (k planes of nV), their sum (1)
 *   SMG_WAVE_ADJ_ADVANCE   x0 = y, x1 = p, x2 = q, x3 = e, x4 = G -> out = p', q', G' (nV x k each)
 *   SMG_WAVE_ADJ_SIGNAL    x0 = y, x1 = gs0, x2 = gs1 (n_idx x k each), idx = the sources -> out = gs0', gs1'
 *   SMG_WAVE_ADJ_SCALE     x0 = G -> out = ((-2.0 mt) / speed) G (nV x k)
 * SMG_ERR_INVALID for an unknown op, nV < 1, nF < 1, a missing operand, k < 1, dt not finite and > 0, clamped not 0 or 1, a speed not finite and
 * > 0, a sigma not finite and >= 0, a face index out of range, n_rows < 1 or n_idx < 1 where they count, a list index out of range, a source
 * listed twice; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_wave_adjoint(int op, int nV, int nF, int k, const int *F, const double *V, const double *speed, const double *sigma, int clamped, double dt,
                           const double *x0, const double *x1, const double *x2, const double *x3, const double *x4, const int *idx, int n_idx, int n_rows,
                           double *out, int *guard_hits);
/* The launcher of the tangent (Born) run's distributed source (csrc/smg_wave_born_device.hip), handle-free and guarded like the hooks above.  F,
 * clamped: the known mask, 1 on the boundary vertices where clamped, as smg_debug_wave derives it.  b, e: nV x k column-major; fd: nV x d_cols,
 * d_cols 1 or k; every array is host.  out = b' (nV x k: b + fd[:, c % d_cols] e off the known rows, b on them), the squares (k planes of nV: 0.0
 * on the known rows, where the kernel leaves what k_wave_rhs wrote), their fixed-order sum (1).
 * SMG_ERR_INVALID, in this order, for nV < 1, nF < 1, F or out missing; a missing operand; k < 1; d_cols not 1 or k; clamped not 0 or 1; a face
 * index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_wave_born(int nV, int nF, int k, int d_cols, const int *F, int clamped, const double *b, const double *e, const double *fd, double *out,
                        int *guard_hits);
/* The time of one launcher of the wave object alone, for tools/wave_time.py: SMG_WAVE_RHS or SMG_WAVE_ADVANCE (with the next right-hand side) on
 * device blocks of zeros of k columns over the mesh (F, V: host), launched `reps` times back to back on one stream between two events after one
 * launch that is not timed; *ms = the mean time of a launch in milliseconds.  SMG_ERR_INVALID for another op, nV < 1, nF < 1, a missing array,
 * k < 1, reps < 1, a face index out of range; SMG_ERR_NO_DEVICE without a GPU. */
int smg_debug_wave_time(int op, int nV, int nF, int k, const int *F, const double *V, int reps, double *ms);

/* One launcher of the union handles (csrc/smg_union_device.hip: smg_hierarchy_create_union), handle-free and guarded like the hooks above.
 * Blocks are row-major n x k, as the solve keeps them; every non-const array is in/out (uploaded, then copied back).  m members.
 *   SMG_UNION_SUMSQ_DECIDE  rptr[m + 1], rows (member i's rows of the block: rows[rptr[i] .. rptr[i + 1]), each row at most once), r, u, zsave,
 *                           ss[m], mdone[m], nhis[m], his (m x cap, cap >= 1), tol and the control block
 *                           -> zsave = u on the listed rows, ss[i] = the member's sum of r^2, every member's break test (mdone, nhis, his) and the
 *                           handle's (the control block)
 *   SMG_UNION_RESTORE       rptr, rows, u, zsave, mdone -> u = zsave on the rows of the members with mdone != 0
 *   SMG_UNION_COARSE        Ainv (the members' dense blocks: block i at moff[i], mlda[i] x mlda[i] row-major), moff[m], mlda[m], mrow0[m + 1],
 *                           row_member[n], b, u -> u[row] += (block of row_member[row])[row - mrow0[i], :] b[mrow0[i] ..]
 * The control block: ctrl_i = {n_his, status, his_cap, -} and ctrl_d = {r_last, -, -} on entry (SUMSQ_DECIDE only; the other ops start from
 * zeros), `done` as given; on return ctrl_i = {n_his, status, his_cap, done}, ctrl_d = {r_last, r_prev, sumsq}; r_his: its history, his_cap
 * entries, in/out.  SMG_ERR_INVALID, before any launch, for an unknown op, m < 1, k < 1, a missing operand, a row outside [0, n) or listed
 * twice, rptr / mrow0 that do not start at 0 or are not monotone, mrow0[m] != n, a row_member that disagrees with mrow0, an mlda that is no
 * multiple of 64 or smaller than its member, an odd or negative moff; SMG_ERR_NO_DEVICE without a GPU. */
enum { SMG_UNION_SUMSQ_DECIDE = 0, SMG_UNION_RESTORE = 1, SMG_UNION_COARSE = 2 };
int smg_debug_union(int op, int m, int n, int k, const int *rptr, const int *rows, double *r, double *u, double *zsave, double *ss, int *mdone,
                    int *nhis, double *his, int cap, const double *Ainv, const long long *moff, const int *mlda, const int *mrow0,
                    const int *row_member, double *b, double tol, int done, double *ctrl_d, int *ctrl_i, double *r_his, int *guard_hits);

/* ---- profc.h mirror: named scopes accumulated with hipEvents (src/profc.h:9-13; mg_VCycle.cpp:121) ------------- */
int smg_prof_enable(smg_hierarchy *h, int on);     /* forces eager launches while on */
int smg_prof_reset(smg_hierarchy *h);
int smg_prof_count(smg_hierarchy *h);
int smg_prof_get(smg_hierarchy *h, int idx, char *name, int name_cap, long *count, double *total_ms);

/* ---- caller-side mesh numerics (host C++; libigl stand-ins used by the demos around the solve) ----------------- */
int smg_mesh_read(const char *path, double **V, int *nV, int **F, int *nF);   /* free with smg_free */
void smg_free(void *p);
int smg_mesh_normalize_unit_area(double *V, int nV, const int *F, int nF);        /* src/normalize_unit_area.cpp */
/* cotmatrix (negative semi-definite, igl convention).  Query nnz with NULL arrays, then fill. */
int smg_mesh_cotmatrix(const double *V, int nV, const int *F, int nF, int *nnz, int *rowptr, int *col, double *val);
int smg_mesh_massmatrix(const double *V, int nV, const int *F, int nF, int voronoi, double *diag);
int smg_mesh_boundary_loop(const int *F, int nF, int nV, int *loop, int *n_loop); /* longest loop; loop holds <= nV */
/* N(f): per face the faces that share at least one vertex with it, without f, as CSR with ascending, duplicate-free rows (ptr: nF + 1 ints).
 * Returns the number of entries (>= 0; with ptr and idx NULL only that: the size query) or a negative error code. */
int smg_mesh_face_neighbours(const int *F, int nF, int nV, int *ptr, int *idx);
/* Lays a flat disk metric out in the plane, host only.  len: nF x 3, the length of the edge opposite every corner (what smg_conformal_lengths
 * returns); X: nV x 2.  Faces are unfolded one after the other in breadth-first order from face 0 (the neighbours across the edges opposite
 * corners 0, 1, 2 in turn): vertex F[0][0] goes to the origin, F[0][1] onto the +x axis, and a vertex is placed once, by the first face that
 * reaches it, to the left of the directed shared edge; a vertex in no face stays at the origin.  stats (2 doubles): the largest relative
 * mismatch between len and the laid-out edge lengths over all faces, and the number of faces of non-positive signed area.  The mismatch is the
 * check: it is the metric's angle defect times the conditioning of the unfolding (errors add up along the breadth-first paths), so a metric
 * that is not flat, or flat but extremely distorted, shows there and not as an error code.  Cutting a closed mesh into a disk is the caller's
 * business.  SMG_ERR_INVALID for a missing array, a face index out of range, a non-finite length, lengths that break the triangle inequality,
 * a face that repeats a vertex, a directed edge that occurs twice (a non-manifold edge or inconsistent orientation), and faces that are not
 * reached across edges from face 0 (more than one component). */
int smg_mesh_unfold(const int *F, int nF, int nV, const double *len, double *X, double *stats);
/* one mid-point upsampling step: S is (nV+nE) x nV in CSR (nV + 2 nE entries), NF is 4 nF x 3 */
int smg_mesh_midpoint_upsample(int nV, const int *F, int nF, int *nE, int *S_rowptr, int *S_col, double *S_val,
                               int *NF);
int smg_mesh_torus(int nu, int nv, double R, double r, double *V, int *F);    /* V: nu*nv x 3, F: 2*nu*nv x 3 */

#ifdef __cplusplus
}
#endif
#endif
