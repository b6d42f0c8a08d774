// smg_device.hpp -- launch interface of the hand-written gfx950 kernels (smg_device.hip).
//
// All dense blocks on the device use the INTERNAL layout: row-major n x k (the k right-hand-side columns
// of one vertex are contiguous, so every neighbour gather is one k*8-byte segment), rows in the level's
// colour-major internal numbering (smg_order.hpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <type_traits>

namespace smg {

// Precision is a type: every view below that holds an fp64 member and its fp32 image hands out the one of type T through an accessor
// (vals<T>() and the like), and this is the one place that says which is which.
template <typename T, typename D, typename F>
constexpr auto by_type(D d, F f) { if constexpr (std::is_same<T, double>::value) return d; else return f; }

// Solve-loop control block, resident in HBM.  The outer loop of min_quad_with_fixed_mg_solve
// (reference src/min_quad_with_fixed_mg.cpp:108-125) is enqueued without host round trips: the decide
// kernel appends to r_his and raises `done`; every later kernel of the stream starts with `if (done) return`.
struct Ctrl {
    int done;      // 1 once residual < tol (or non-finite) was observed
    int n_his;     // entries of r_his written
    int status;    // 0 ok, -1 non-finite residual
    int just_done; // set by the speculative decide when this very decision ended the loop
    double sumsq;  // sum of squares of the last residual (all-reduced across ranks when column-sharded)
    double tol;    // absolute tolerance of the break test (kept here so captured graphs do not bake it in)
    double* r_his; // residual history in HBM, his_cap entries (sized from max_iter at smg_solve_begin; read through this
    int his_cap;   // pointer at run time, so captured graphs survive a re-allocation)
    int pad_;
    double r_last, r_prev;   // the two most recent residuals (what the host's adaptive polling extrapolates from)
};

struct SellDev {
    int n_rows = 0, n_cols = 0, n_slices = 0;
    int C = 64;                      // slice height: 64 (one row per lane) or 128 (two adjacent rows per lane)
    const int* slice_row = nullptr;  // n_slices + 1
    const int* slice_off = nullptr;  // n_slices + 1 (units of C entries); = s * stride when stride > 0
    const int* slice_w = nullptr;    // n_slices: panel columns used by the slice
    int stride = 0;                  // > 0: fixed panel pitch, addressing needs no table
    int w_lo = 0;                    // columns requested before the slice's width is known, <= stride (0 when stride == 0)
    int w_max = 0;                   // widest slice (panel columns)
    const int* order = nullptr;      // optional launch order of the slices (region-major), whole-matrix kernels only
    const int* col = nullptr;
    const double* val = nullptr;
    const float* valf = nullptr;     // fp32 copy of val (same slots), only for the mixed-precision V-cycle
    // Weight codes (transfer operators of subdivision hierarchies: P holds 1.0 and 0.5 only): codes != 0 means there is no value array
    // (val / valf are null); every stored slot's column word is (column << 2) | code and its value is tab[code] (tabf: the fp32 image).
    // Padding stays -1 (an arithmetic shift by 2 keeps it -1).  SellBuf::encode_codes builds it; smg_device.hip decodes it.
    int codes = 0;
    double tab[4] = {0.0, 0.0, 0.0, 0.0};
    float tabf[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // Long rows taken out of the panels (restriction operators of decimated hierarchies: a coarse vertex of the reference's construction
    // may gather from > 100 fine ones, and a panel row is one chain of dependent batches -- it set the launch's duration): in CSR,
    // ascending column order, served by launch_sell(SELL_AX) through a companion launch of one wave per (row, column); the panels hold
    // these rows empty.  Same products, same order of additions: bit-identical.
    int long_n = 0;
    const int* long_row = nullptr;   // long_n row numbers
    const int* long_ptr = nullptr;   // long_n + 1
    const int* long_col = nullptr;
    const double* long_val = nullptr;
    const float* long_valf = nullptr;
    template <typename T> const T* vals() const { return by_type<T>(val, valf); }
    template <typename T> const T* long_vals() const { return by_type<T>(long_val, long_valf); }
    template <typename T> const T* table() const { return by_type<T>(tab, tabf); }
};

enum SellMode {
    SELL_AX = 0,        // y = A x                       (mg_VCycle.cpp:69 `A`, :91 `prolong`, :80 `restrict`)
    SELL_RESID = 1,     // y = b - A x                   (mg_VCycle.cpp:41-42)
    SELL_RESID_SS = 2,  // partial sums of |b - A x|^2   (min_quad_with_fixed_mg.cpp:110 / :332)
    SELL_ADD = 3,       // y = y + A x                   (mg_VCycle.cpp:51-53  u = u + P uc)
    SELL_GS = 4,        // y_i = (b_i - sum_{j != i} A_ij y_j) / A_ii on the given slice range (one colour)
    SELL_RESID_BOTH = 5,  // y = b - A x AND the partial sums of its squares (outer loop of the mixed-precision mode)
    SELL_JACOBI = 6,    // y_i = x_i + omega * ((b_i - sum_{j != i} A_ij x_j) / A_ii - x_i): one damped-Jacobi sweep from x into y (x != y),
                        // whole matrix in one launch (the "Jacobi" of BASELINE.json's north_star; same slot as SELL_GS, mg_VCycle.cpp:113-178)
    SELL_CHEBY = 7,     // one step of Chebyshev-accelerated Jacobi from x into y (x != y):  r_i = (b_i - sum_{j != i} A_ij x_j) / A_ii - x_i,
                        // d_i = c1 d_i + c2 r_i (first step, c1 == 0: d_i = c2 r_i, d not read),  y_i = x_i + d_i
    // ---- the outer loop's residual folded into the first smoothing launches of the V-cycle (level 0 only, fp64 only) ----
    // The reference computes |RHS - A z| (min_quad_with_fixed_mg.cpp:110), tests it, and then starts the cycle with relax() on the same
    // z: the first sweep streams the same matrix rows again.  These modes take the squared residual of the OLD iterate out of that
    // sweep -- per row a second accumulator, b_i - sum_j A_ij x_j over ALL stored entries in slot order, bit for bit what SELL_RESID_SS
    // forms -- and write the sweep's result OUT OF PLACE (y != x), so that the old iterate survives when the break test says stop.
    SELL_GS_OOP = 8,      // one colour of a Gauss-Seidel sweep from x into y: neighbours in earlier colours (rows below the first row of
                          // the launch's slice range: colour-major numbering) are read from y, the others from x.  Same values, same order
                          // as the in-place launch.
    SELL_GS_HEAD = 9,     // SELL_GS_OOP + partial sums of |b - A x|^2 over the rows of the colour
    SELL_JACOBI_HEAD = 10,  // SELL_JACOBI + partial sums of |b - A x|^2
    SELL_CHEBY_HEAD = 11,   // SELL_CHEBY + partial sums of |b - A x|^2
    // ---- the level residual of the V-cycle as a by-product of the LAST colour launch of the pre-smoothing (fp64, k < 8, scalar levels) ----
    // After that launch every row of the level is final, and the launch holds every stored entry of its rows, the final iterate at every
    // column and its own new value: it also stores r_i = b_i - sum_j a_ij u_j of its rows into first->d.  The rows of the last colour close
    // the numbering, so the diagonal is the last stored entry of each: the sweep's sum plus diagonal times new value IS SELL_RESID's sum, term
    // by term in slot order -- the same bits.  The slice range must end with the matrix.  The residual launch that follows covers the other
    // colours only (SellBuf::order_part).
    SELL_GS_RES = 12,       // SELL_GS on the last colour + the residual of its rows
    SELL_GS_OOP_RES = 13,   // SELL_GS_OOP on the last colour + the residual of its rows
};
constexpr bool sell_has_res(int m) { return m == SELL_GS_RES || m == SELL_GS_OOP_RES; }
constexpr bool sell_is_gs(int m) { return m == SELL_GS || m == SELL_GS_OOP || m == SELL_GS_HEAD || sell_has_res(m); }
constexpr bool sell_is_oop(int m) { return m == SELL_GS_OOP || m == SELL_GS_HEAD || m == SELL_GS_OOP_RES; }
constexpr bool sell_is_jacobi(int m) { return m == SELL_JACOBI || m == SELL_JACOBI_HEAD; }
constexpr bool sell_is_cheby(int m) { return m == SELL_CHEBY || m == SELL_CHEBY_HEAD; }
constexpr bool sell_is_head(int m) { return m == SELL_GS_HEAD || m == SELL_JACOBI_HEAD || m == SELL_CHEBY_HEAD; }
constexpr bool sell_has_ss(int m) { return sell_is_head(m) || m == SELL_RESID_SS || m == SELL_RESID_BOTH; }
// no fp32 twin: the norms belong to the fp64 outer loop, and the fp32 cycle keeps its whole first sweep and its whole residual launch
constexpr bool sell_fp64_only(int m) { return sell_has_ss(m) || sell_is_oop(m) || sell_has_res(m); }

// SELL_ADD: y = b + A x, where b is the iterate the correction is added to (b == nullptr: in place, b = y).
// y/x/b: internal layout, ld = number of columns k.  Slices [s_begin, s_end).  `ctrl` may be null (no
// early-exit test).  For SELL_RESID_SS, `partials` receives one double per launched block; the number of
// blocks is returned through *n_blocks.
// zero_rows (SELL_AX only, optional): an n_rows x k block that is set to +0.0 row by row alongside y (the restriction
// launch also performs `uc.setZero()`, mg_VCycle.cpp:46-47).
// first (with zero_rows, optional): the rows of the coarse level's first colour get, instead of +0.0, what the first colour
// launch of the first pre-smoothing sweep would leave there -- y_i / a_ii: with a zero initial guess every product of that
// launch is a_ij * 0, so (b_i - 0) / a_ii is bit for bit the sweep's value, and the cycle skips that launch.
struct FirstColour {
    const int* diag_slot = nullptr;   // per row of the first colour: slot of the diagonal in the sweep's SELL value array
    int n_first = 0;                  // rows of the first colour (they lead the colour-major numbering)
    const double* val = nullptr;      // the sweep's SELL values (A or A^T) ...
    const float* valf = nullptr;      // ... and their fp32 image
    int jacobi = 0;                   // 1: the coarse level is smoothed by damped Jacobi: n_first = all its rows, and they receive the
    double omega = 1.0;               //    first sweep from u = 0:  0 + omega * (y_i / a_ii - 0).  2: Chebyshev-Jacobi: d_i = omega * (y_i /
                                      //    a_ii - 0), u_i = 0 + d_i, both written (d / df below)
    double* d = nullptr;              // SELL_CHEBY launches and jacobi == 2: the update vector (n x k, internal layout) ...; SELL_GS_RES /
                                      // SELL_GS_OOP_RES: where the residual of the launch's rows goes
    float* df = nullptr;              // ... its fp32 twin
    double c1 = 0.0;                  // SELL_CHEBY: coefficient of the old update (0 = first step, d is not read); `omega` is c2
    template <typename T> const T* vals() const { return by_type<T>(val, valf); }
    template <typename T> T* update() const { return by_type<T>(d, df); }
    template <typename T> void set_update(T* p) { if constexpr (std::is_same<T, double>::value) d = p; else df = p; }
};
hipError_t launch_sell(SellMode mode, const SellDev& A, int s_begin, int s_end, const double* x, const double* b,
                       double* y, int k, const Ctrl* ctrl, double* partials, int* n_blocks, hipStream_t st,
                       double* zero_rows = nullptr, const FirstColour* first = nullptr, double omega = 1.0);
// the same on the fp32 image (A.valf, or weight codes) for the mixed-precision V-cycle: the modes without a norm, a head or a residual
// by-product (sell_fp64_only), partials == nullptr; anything else is hipErrorInvalidValue
hipError_t launch_sell(SellMode mode, const SellDev& A, int s_begin, int s_end, const float* x, const float* b,
                       float* y, int k, const Ctrl* ctrl, double* partials, int* n_blocks, hipStream_t st,
                       float* zero_rows = nullptr, const FirstColour* first = nullptr, double omega = 1.0);
// *out (device double) = max_i (sum_j |a_ij|) / a_ii over the rows of A: the Gershgorin bound of the spectrum of D^-1 A
hipError_t launch_gershgorin(const SellDev& A, double* out, hipStream_t st);
// ---- block (3 degrees of freedom per vertex) matrices: smg_bsr3.hpp (layout), smg_bsr3_device.hip (kernels) ------------------------
struct Bsr3Dev {
    int n_vert = 0, n_slices = 0, w_max = 0;
    const int* slice_row = nullptr;  // n_slices + 1 vertex offsets
    const int* slice_off = nullptr;  // n_slices + 1 panel-column offsets
    const int* slice_w = nullptr;    // n_slices
    const int* order = nullptr;      // optional region-major launch order, whole-matrix launches only
    const int* col = nullptr;        // block columns (vertices), -1 = padding
    const double* val = nullptr;     // nine planes per panel column
    const float* valf = nullptr;     // ... their fp32 image (mixed-precision cycle), or null
    template <typename T> const T* vals() const { return by_type<T>(val, valf); }
};
// modes SELL_AX, _RESID, _RESID_SS, _GS (one vertex colour = slices [s_begin, s_end), in place: y == x), _JACOBI, _CHEBY with the meaning
// they have per scalar row of the 3n x 3n matrix.  x / b / y / dvec: row-major (3 n_vert) x k.  omega, c1, dvec: as in launch_sell
// (Jacobi damping; Chebyshev: omega = c2, c1, the update vector).  partials / n_blocks: SELL_RESID_SS, one double per launched block.
hipError_t launch_bsr3(SellMode mode, const Bsr3Dev& A, int s_begin, int s_end, const double* x, const double* b, double* y, int k, const Ctrl* ctrl,
                       double* partials, int* n_blocks, hipStream_t st, double omega = 1.0, double c1 = 0.0, double* dvec = nullptr);
// the same on the fp32 image (A.valf; SELL_AX, _RESID, _GS, _JACOBI, _CHEBY, partials == nullptr); SELL_RESID_BOTH (fp64 only, above): y = b - A x and the
// partial sums of its squares
hipError_t launch_bsr3(SellMode mode, const Bsr3Dev& A, int s_begin, int s_end, const float* x, const float* b, float* y, int k, const Ctrl* ctrl,
                       double* partials, int* n_blocks, hipStream_t st, double omega = 1.0, double c1 = 0.0, float* dvec = nullptr);
hipError_t launch_bsr3_gershgorin(const Bsr3Dev& A, double* out, hipStream_t st);
int bsr3_blocks(int n_slices);
// the image B (laid out on the host, Bsr3Buf::upload of a layout; panel_cols = its panel columns) filled on the device from the scalar CSR arrays of A
// in the caller's numbering, the pattern of its blocks (gptr / gcol) and the vertex numbering (perm new -> old, iperm): B = A(perm3, perm3), or its
// transpose (A structurally symmetric)
hipError_t launch_bsr3_fill(const int* ptr, const int* col, const double* val, const int* gptr, const int* gcol, const int* perm, const int* iperm, const Bsr3Dev& B,
                            size_t panel_cols, bool transposed, hipStream_t st);

// ---- Gauss-Seidel sweep for blocks of 64 right-hand-side columns: block-sequential order (smg_bgs.hpp plan, smg_bgs_device.hip kernel) ----
struct BgsDev {
    int n_blocks = 0, n_colors = 0, xrows = 0;   // xrows: rows of a block's LDS image (own rows + the level's largest rim, a multiple of 128)
    const int* hdr = nullptr;         // per block BGS_HDR ints: first unit, units, batches per row, first entry slot, local rows in use
    const int* xrow = nullptr;        // xrows per block: the row behind local index l (own rows, then the rim)
    const int* ugrow = nullptr;       // 16 per unit: row, ...
    const int* ulrow = nullptr;       //   ... its local index, ...
    const double* udiag = nullptr;    //   ... its diagonal entry
    const int* eidx = nullptr;        // 16 x 8 NB per unit: local index of the entry's column
    const double* eval = nullptr;     //   ... its value
};
// the blocks [b_begin, b_end) -- one block colour -- of one sweep, in place on u (row-major n x k, k a multiple of 16)
hipError_t launch_bgs(const BgsDev& P, int b_begin, int b_end, const double* b, double* u, int k, const Ctrl* ctrl, hipStream_t st);

// ---- Gauss-Seidel sweep of a Galerkin level of a decimated hierarchy: one wavefront per piece, one launch per piece colour (smg_wgs.hpp plan, smg_wgs_device.hip kernel) ----
struct WgsDev {
    int n_pieces = 0, n_colors = 0, rim_pitch = 0, nb_max = 0;   // nb_max: batches of 8 entry slots of the level's widest row
    const int* hdr = nullptr;         // per piece WGS_HDR ints: first entry slot, batches per row, rim rows, phases, ...
    const int* grow = nullptr;        // 64 per piece: the lane's row (-1: none), ...
    const int* meta = nullptr;        //   ... the phase it is updated in | batches its row needs << 16, ...
    const double* diag = nullptr;     //   ... its diagonal entry
    const int* rim = nullptr;         // rim_pitch per piece: the rows behind local indices 64, 65, ...
    const unsigned* eoff = nullptr;   // per piece 64 x 4 NB: byte offsets of two entry slots' columns in the one-column image, 16 + 16 bits
    const double* eval = nullptr;     // per piece 64 x 8 NB: the values
};
// the pieces [q_begin, q_end) -- one piece colour -- of one sweep, in place on u (row-major n x k, any k >= 1: column groups ride in the grid's second dimension)
hipError_t launch_wgs(const WgsDev& P, int q_begin, int q_end, const double* b, double* u, int k, const Ctrl* ctrl, hipStream_t st);
// what launch_wgs decides, and nothing else decides it: the kernel's row-width class NBMAX (3 / 5 / 8) and rim slots per lane RIMI (2 / 4 / 7) of a
// plan (false: no variant), and the launch -- `groups` groups of kb columns per lane -- that serves columns c0 ... of k on a level of n_pieces pieces
bool wgs_kernel_class(int nb_max, int rim_pitch, int* nbmax, int* rimi);
void wgs_column_split(int n_pieces, int k, int c0, int* kb, int* groups);

// ---- independent meshes in one handle (smg_hierarchy_create_union; kernels: smg_union_device.hip) ----
struct UnionDev {
    int m = 0, his_cap = 0, max_rows = 0;      // members; entries per member history; rows of the largest member on level 0
    const int* rows = nullptr;                 // level 0: internal row numbers grouped by member ...
    const int* rptr = nullptr;                 // ... m + 1 offsets
    const int* crow_member = nullptr;          // coarsest level: row -> member
    const long long* moff = nullptr;           // per member: offset of its inverse in the handle's d_Ainv
    const int* mlda = nullptr;                 // ... its leading dimension (rows padded to 64)
    const int* mrow0 = nullptr;                // ... its first row on the coarsest level
    double* ss = nullptr;                      // m: sum of squares of the member's residual
    double* his = nullptr;                     // m x his_cap: the members' residual histories
    int* nhis = nullptr;                       // m: entries written
    int* done = nullptr;                       // m: the member's loop has ended
    double* zsave = nullptr;                   // n_0 x k: the iterate before the cycle
};
// u[:, c] += blockdiag(Ainv_i) b[:, c] on the coarsest level (n rows in all)
hipError_t launch_blockdiag_gemv_add(const UnionDev& U, const double* Ainv, int n, const double* b, double* u, int k, const Ctrl* ctrl, hipStream_t st);
// per member: ss = |r|^2 over its rows, zsave = u there; then every member's break test and the handle's (ctrl): done when all members are
hipError_t launch_union_sumsq_decide(const UnionDev& U, const double* r, const double* u, int k, Ctrl* ctrl, hipStream_t st);
// after a cycle: members whose loop has ended get their rows of zsave back
hipError_t launch_union_restore(const UnionDev& U, double* u, int k, const Ctrl* ctrl, hipStream_t st);
hipError_t launch_scatter_dense(double* dense, const double* src, const long long* pos, int nnz, hipStream_t st);
hipError_t launch_dense_identity(double* dense, int np, int n, hipStream_t st);

// ---- relax(iters) of a latency-bound level in one launch: overlapped tiling (smg_tiled.hpp plan, smg_tiled_device.hip kernel) ------
struct TiledDev {
    int n_tiles = 0, nc = 0, P = 0, sweeps = 0, max_ext = 0, w_max = 0, threads = 512;
    const int* hdr = nullptr;
    const int* ext_rows = nullptr;
    const int* pcol = nullptr;
    const double* pval = nullptr;
    const int* prow = nullptr;
    const double* pdiag = nullptr;     // like prow: the diagonal entry of every panel row (its slot in the panel holds +0.0)
};
// y = relax(sweeps) of x with right-hand side b, x != y, row-major n x k blocks
hipError_t launch_tiled_gs(const TiledDev& T, const double* x, const double* b, double* y, int k, const Ctrl* ctrl, hipStream_t st);
hipError_t tiled_gs_prepare(int max_ext);

// ---- sparse coarse solver (smg_coarse.hpp): P A P^T = L L^T factored on the host, the triangular solves here --------------------------
struct SparseCholDev {
    int n = 0;
    const int* perm = nullptr;                       // new -> old
    const int *rptr = nullptr, *rcol = nullptr;      // strict lower triangle by rows
    const int *cptr = nullptr, *crow = nullptr;      // ... and by columns
    const double *rval = nullptr, *cval = nullptr, *diag = nullptr;
    double* work = nullptr;                          // 2 n KC (KC = columns per pass, sparse_coarse_work_cols): the forward solve's z, the backward solve's x
    int* err = nullptr;                              // [0] raised when a wait gave up; [1], [2]: ticket counters of the forward / backward launch
};
// u[:, c] += (L L^T)^-1 b[:, c] for the k columns of the row-major n x k blocks (caller numbering of the coarsest level)
hipError_t launch_sparse_coarse_solve(const SparseCholDev& F, const double* b, double* u, int k, const Ctrl* ctrl, hipStream_t st);
int sparse_coarse_work_cols(int k);   // F.work must hold 2 n sparse_coarse_work_cols(k) doubles for a solve with k columns

// ---- Schur-complement coarse solver (smg_schur.hpp): interior blocks of <= 64 rows eliminated exactly, the separator inverted densely ----
constexpr int SCHUR_M_MAX_DEV = 128;                 // = SCHUR_M_MAX (smg_schur.hpp): separator rows a block touches at most
struct SchurDev {
    int n = 0, nb = 0, ns = 0, ns_pad = 0;
    const int *irow = nullptr, *bsize = nullptr, *srow = nullptr, *sptr = nullptr, *sidx = nullptr, *aptr = nullptr, *ablk = nullptr, *apan = nullptr;
    double* arena = nullptr;                         // [D^-1 blocks][P^T panels][W^T panels][S^-1][products]: smg_schur.hpp
    float* arena32 = nullptr;                        // fp32 image of the arena (mixed-precision cycle), or null
    long long off_D = 0, off_P = 0, off_W = 0, off_S = 0, off_C = 0;
    const long long *coff = nullptr, *pos = nullptr, *pos2 = nullptr, *ones = nullptr, *rdst = nullptr, *rdst2 = nullptr, *rsrc = nullptr;
    const int* rptr = nullptr;
    int nnz = 0, n_ones = 0, n_red = 0;
    double *g = nullptr, *xs = nullptr;              // ns_pad x k each: the separator's right-hand side and solution
    float *g32 = nullptr, *xs32 = nullptr;
    double* sym_work = nullptr;                      // (ns_pad / 64)^2 x 64: the k = 1 product with S^-1 through its lower triangle
    double* gj_work = nullptr;                       // launch_spd_inverse's scratch for ns_pad
    template <typename T> const T* factors() const { return by_type<T>(arena, arena32); }
    template <typename T> T* rhs() const { return by_type<T>(g, g32); }
    template <typename T> T* sol() const { return by_type<T>(xs, xs32); }
};
// arena <- the factorisation of the matrix whose values (CSR order of the plan's matrix) are vals
hipError_t launch_schur_factor(const SchurDev& F, const double* vals, hipStream_t st);
// *d_flag = 1 when the factorisation in the arena cannot be that of an SPD matrix (a non-positive or non-finite diagonal entry of an inverse), else 0
hipError_t launch_schur_check(const SchurDev& F, int* d_flag, hipStream_t st);
// u[:, c] += A^-1 b[:, c] for the k columns of the row-major n x k blocks (caller numbering of the coarsest level)
hipError_t launch_schur_solve(const SchurDev& F, const double* b, double* u, int k, const Ctrl* ctrl, hipStream_t st);
hipError_t launch_schur_solve(const SchurDev& F, const float* b, float* u, int k, const Ctrl* ctrl, hipStream_t st);   // on arena32 / g32 / xs32

int sell_blocks(int n_slices);  // 4 slices (waves) per 256-thread block
int sell_wide_blocks(int n_slices, int k);  // partial-sum slots the wide (k >= 8) path needs
// The k_sell_deep launches (smg_device.hip) that serve a narrow group of kb <= 4 fp64 columns of mode (SELL_AX / SELL_RESID) on a matrix whose widest
// row has w_max entries: columns per launch in cols[0 .. return value), *nbmax the kernel's row-width class (3 / 5 / 8); 0: k_sell serves the group
int deep_split(int mode, int w_max, int kb, int* cols, int* nbmax);
int gs_colour_wpb(const SellDev& A, int n_slices);  // waves per workgroup (2 / 4 / 8) of a one-column Gauss-Seidel colour launch of n_slices slices of A
bool wide_latency_variant(int n_slices, int kw);  // a wide launch of n_slices slices, kw < 64 columns: one row per lane (true) or the streaming kernel

// ctrl->sumsq = sum(partials[0..n)) in a fixed order (deterministic).  The buffer must have ss_partials_room() doubles of room behind the n partials
// (large n: a first launch leaves per-share sums there).
int ss_partials_room();
// ctrl->sumsq = sum(partials[0..n)) in a fixed order (deterministic).
hipError_t launch_ss_finalize(const double* partials, int n, Ctrl* ctrl, hipStream_t st, double* out = nullptr);   // out: where the sum goes (default ctrl->sumsq)
// r = sqrt(*sumsq); append to r_his; done = (r < ctrl->tol) or non-finite.  No-op when already done.
hipError_t launch_decide(Ctrl* ctrl, const double* sumsq, hipStream_t st);
// speculative split-phase iteration (the V-cycle overlaps the all-reduce): see smg.h, smg_solve_iter_cycle_speculative
hipError_t launch_decide_spec(Ctrl* ctrl, const double* sumsq, hipStream_t st);
hipError_t launch_copy_unless_done(double* dst, const double* src, size_t n, const Ctrl* ctrl, hipStream_t st);
hipError_t launch_restore_if_just_done(double* dst, const double* src, size_t n, const Ctrl* ctrl, hipStream_t st);
// both of the above in one launch (single-GPU path, no all-reduce in between)
hipError_t launch_ss_finalize_decide(const double* partials, int n, Ctrl* ctrl, hipStream_t st);

// ---- conjugate gradients preconditioned by the V-cycle (smg_solve_pcg; kernels: smg_krylov_device.hip) --------------------------------
// Per-column scalars of the recurrence: s[slot * k + c]
enum { KS_RZ = 0, KS_RZ_PREV = 1, KS_ALPHA = 2, KS_BETA = 3, KS_SLOTS = 4 };
constexpr int KRY_MAX_GROUPS = 512;
struct KryDev {
    int n = 0, k = 0;            // the internal blocks: row-major n x k
    int groups = 0;              // row chunks of the reduction launches (kry_groups(n, k))
    double* part = nullptr;      // 2 x groups x k partial sums
    double* s = nullptr;         // KS_SLOTS x k
    int* restart = nullptr;      // 1: the next direction is z itself (first iteration, or a restart from the true residual)
};
int kry_groups(int n, int k);
// rz_c = z.r and beta_c = -alpha_c (z.q)_c / rz_prev_c (the flexible, Polak-Ribiere form: z.(r_new - r_old) / rz_prev, as r_old - r_new = alpha q)
hipError_t launch_kry_dots_zr_zq(const KryDev& K, const double* z, const double* r, const double* q, const Ctrl* ctrl, hipStream_t st);
// p = z + beta_c p
hipError_t launch_kry_direction(const KryDev& K, const double* z, double* p, const Ctrl* ctrl, hipStream_t st);
// alpha_c = rz_c / (p.q)_c, rz_prev_c = rz_c
hipError_t launch_kry_dots_pq(const KryDev& K, const double* p, const double* q, const Ctrl* ctrl, hipStream_t st);
// x += alpha_c p, r -= alpha_c q, then |r|_F -> the history and the break test (as launch_decide)
hipError_t launch_kry_step_decide(const KryDev& K, double* x, double* r, const double* p, const double* q, Ctrl* ctrl, hipStream_t st);
// b0 = r, u0 = 0: the fp64 preconditioner's input;  z = (double) e: the fp32 one's output
hipError_t launch_kry_precond_in(const double* r, double* b0, double* u0, size_t cnt, const Ctrl* ctrl, hipStream_t st);
hipError_t launch_kry_widen(const float* e, double* z, size_t cnt, const Ctrl* ctrl, hipStream_t st);
// restart flag = 1; reopen: also lower `done` and drop the last history entry (the host's check of a recurrence norm replaces it by the true one)
hipError_t launch_kry_arm(const KryDev& K, Ctrl* ctrl, bool reopen, hipStream_t st);

// ---- LOBPCG eigensolver (smg_eigs, host side smg_eig.cpp; kernels: smg_eig_device.hip) ------------------------------------------------
// The basis S = [X W P] is up to three row-major n x m blocks (m <= 64 columns each), concatenated by columns: column i of S is column i % m
// of block i / m.  Every kernel returns at once when ctrl->done is set, as the V-cycle's do.
struct EigBlocks {
    const double* p[3] = {nullptr, nullptr, nullptr};
    int nb = 0;                  // blocks in use
};
constexpr int EIG_TILE = 64;            // Gram output tile (EIG_TILE x EIG_TILE entries per work-group)
constexpr int EIG_MAX_GROUPS = 256;
int eig_groups(int n);                  // row chunks of the reductions: a function of n alone (determinism)
// the partial-sum room the Gram of an a x b product needs (doubles), for groups = eig_groups(n)
size_t eig_gram_part_size(int a, int b, int groups);
// G (row-major a x b, a = Sa.nb * m, b = Sb.nb * m) = Sa^T diag(w) Sb; w == nullptr: 1.  sym (Sa == Sb): only the tiles on and above the
// diagonal are formed, the finalize mirrors them (G exactly symmetric).  Fixed row chunks, one partial per chunk, summed in chunk order.
hipError_t launch_eig_gram(const EigBlocks& Sa, const EigBlocks& Sb, int n, int m, const double* w, bool sym, double* part, int groups,
                           double* G, const Ctrl* ctrl, hipStream_t st);
// With C row-major q x 2m (q = S.nb * m; columns 0..m-1: Cx, m..2m-1: Cp):  X = S Cx, AX = AS Cx and, when P != nullptr, P = S' Cp,
// AP = AS' Cp where S' leaves out block 0 (the X rows of Cp are not read).  Outputs must not alias the inputs.
hipError_t launch_eig_combine(const EigBlocks& S, const EigBlocks& AS, int n, int m, const double* C, double* X, double* AX, double* P,
                              double* AP, const Ctrl* ctrl, hipStream_t st);
// R = AX - diag(mass) X diag(lam); res_c = sqrt(sum_i r_ic^2 / mass_i) / |lam_c|.  The preconditioner's input in the same pass:
// b32 == nullptr: b0 = R, u0 = 0 (fp64 cycle); else b32 = (float) R, u32 = 0 (fp32 cycle).
hipError_t launch_eig_residual(const double* X, const double* AX, const double* mass, const double* lam, int n, int m, double* b0, double* u0,
                               float* b32, float* u32, double* part, int groups, double* res, const Ctrl* ctrl, hipStream_t st);

// u[i,:] += sum_j Ainv[i,j] * b[j,:]   (mg_VCycle.cpp:199-200 with the factorisation pre-inverted)
// sym_work (optional, (lda/64)^2 * 64 elements): with it, a single column (k = 1) is multiplied through the lower triangle of
// tiles only (the inverse is symmetric): half the bytes, two launches, deterministic per-row summation in block order.
// b, u: row-major n x ld blocks of which the first k columns take part (ld >= k)
hipError_t launch_dense_gemv_add(const double* Ainv, int n, int lda, const double* b, double* u, int k, int ld,
                                 const Ctrl* ctrl, hipStream_t st, double* sym_work = nullptr);
hipError_t launch_dense_gemv_add(const float* Ainv, int n, int lda, const float* b, float* u, int k, int ld,
                                 const Ctrl* ctrl, hipStream_t st, float* sym_work = nullptr);
// first half of the symmetric k = 1 product alone: part[(I * (lda / 64) + J) * 64 + r] = the share of tile (I, J) in row 64 I + r of Ainv b; lda % 64 == 0
hipError_t launch_sym_gemv_tiles(const double* Ainv, int lda, const double* b, double* part, hipStream_t st);
hipError_t launch_sym_gemv_tiles(const float* Ainv, int lda, const float* b, float* part, hipStream_t st);
// mixed precision glue
hipError_t launch_cvt_f64_f32(float* dst, const double* src, size_t n, hipStream_t st);
hipError_t launch_residual_to_f32(float* b32, float* u32, const double* r64, size_t n, const Ctrl* ctrl, hipStream_t st);
hipError_t launch_add_correction(double* z, const float* e, size_t n, const Ctrl* ctrl, hipStream_t st);
// In-place inversion of an SPD matrix (n x n, row-major, leading dimension lda, n % 64 == 0, lda == n) by
// blocked Gauss-Jordan elimination without pivoting.  work: 2*n*64 + 2*64*64 doubles.
hipError_t launch_spd_inverse(double* M, int n, double* work, hipStream_t st);

// value-only re-precompute (same sparsity as the last full precompute) -------------------------------------------
// out[e] = sum_t coef[t] * src[idx[t]]  (numeric Galerkin stage with a fixed recipe, smg_sparse.hpp)
hipError_t launch_recipe(int n_out, const int* ptr, const int* idx, const double* coef, const double* src, double* out, hipStream_t st);
// SELL panels of A(perm, perm) from A's CSR arrays (caller numbering, on the device): S.col / S.val (padded slots) are cleared and filled
// transposed: the image of A(perm, perm)^T instead -- A structurally symmetric (launch_bit_symmetric), values looked up by bisection
hipError_t launch_sell_fill(const int* ptr, const int* col, const double* val, const int* perm, const int* iperm, const SellDev& S, size_t padded, hipStream_t st,
                            bool transposed = false);
// out_col[i] = S.col[i] < 0 ? -1 : (S.col[i] << 2) | code, where tab[code] is bit for bit S.val[i] (n_tab <= 4 entries); *bad (preset to 0 by
// the caller) is raised when a stored slot's value is not in the table or its column does not fit in 29 bits
hipError_t launch_sell_encode(const SellDev& S, size_t padded, const double* tab, int n_tab, int* out_col, int* bad, hipStream_t st);
// slot[r] = index of a_rr in the value array of the filled square image S (-1: not stored); *first_missing (preset to n_rows by the caller) =
// the smallest row without one
hipError_t launch_sell_diag_slots(const SellDev& S, int* slot, int* first_missing, hipStream_t st);
// one empty launch: makes the runtime load this library's main code object now rather than inside the first real launch
hipError_t warm_device_code(hipStream_t st);
// map[slot] = index of the CSR entry slot holds in the image launch_sell_fill(..., transposed) builds (-1: padding): the gather map of
// the value-only re-precompute, for an image of that layout however it was built
hipError_t launch_sell_fill_map(const int* ptr, const int* col, const int* perm, const int* iperm, const SellDev& S, size_t padded, bool transposed, int* map, hipStream_t st);
// square CSR matrix (rows sorted) on the device: *differs = 0 when A == A^T bit for bit; bit 0: some value differs from its mirror image,
// bit 1: some entry has none (A is not structurally symmetric)
hipError_t launch_bit_symmetric(int n, const int* ptr, const int* col, const double* val, int* differs, hipStream_t st);
// dst[i] = map[i] >= 0 ? src[map[i]] : 0   (refresh of SELL value panels / LHS and Auk slices)
hipError_t launch_gather_vals(double* dst, const double* src, const int* map, size_t n, hipStream_t st);
// dense (np x np, row-major) = identity on the padding rows, zero elsewhere, then dense[pos[i]] = src[i]
hipError_t launch_dense_from_csr(double* dense, int np, int n, const double* src, const long long* pos, int nnz, hipStream_t st);
hipError_t launch_add_at(double* v, const int* where, int n, double c, hipStream_t st);

// operator assembly on the device for a fixed connectivity (row f-3): per-face terms, lumped mass, CSR values
// val = mass_coef * M + lap_coef * L  (L = igl::cotmatrix convention); Lval (optional) receives L alone.
hipError_t launch_assemble(int nV, int nF, int nnz, const double* V, const int* F, int voronoi, const int* l_ptr, const int* l_idx,
                           const signed char* l_sgn, const int* m_ptr, const int* m_idx, const int* diag_of, double* Qc, double* Qm,
                           double* Md, double mass_coef, double lap_coef, double* val, double* Lval, hipStream_t st);

// layout helpers ------------------------------------------------------------------------------------------
// dst[i*kin + c] = c < k ? src[map[i] + c*ld_src] : 0      (column-major caller block -> internal block of kin >= k columns per row)
hipError_t launch_gather_in(double* dst, const double* src, const int* map, int n, int k, int kin, int ld_src,
                            hipStream_t st);
// dst[map[i] + c*ld_dst] = src[i*kin + c], c < k
hipError_t launch_scatter_out(double* dst, const double* src, const int* map, int n, int k, int kin, int ld_dst,
                              hipStream_t st);
// dst[idx[i] + c*ld_dst] = src[i + c*ld_src]  (column-major -> column-major scatter, known values)
hipError_t launch_scatter_cm(double* dst, const double* src, const int* idx, int n, int k, int ld_src, int ld_dst,
                             hipStream_t st);
// dst[i + c*ld_dst] = src[idx[i] + c*ld_src]  (column-major row gather, igl::slice(X, idx, 1, Y))
hipError_t launch_gather_cm(double* dst, const double* src, const int* idx, int n, int k, int ld_src, int ld_dst,
                            hipStream_t st);
// y[i + c*ld] -= sum_p val[p] * x[col[p] + c*ldx]   (CSR, column-major blocks; RHS_u -= Auk * known_val,
// min_quad_with_fixed_mg.cpp:318.  The product is summed first, then subtracted.)
hipError_t launch_csr_sub(int n_rows, const int* ptr, const int* col, const double* val, const double* x, int ldx,
                          double* y, int ld, int k, hipStream_t st);

// heat-method geodesics (smg_geodesics_device.hip; column-major caller blocks, column c of vertex i at c * ld + i) -------------------
// W[9f + 3i + d] = ((n x e_i) / (2A))_d, the gradient of corner i's hat function on face f; Af[f] = A (V: nV x 3 row-major)
hipError_t launch_geo_basis(const double* V, const int* F, int nF, double* W, double* Af, hipStream_t st);
// B = the n x k indicator block: 1 at the sources src[src_ptr[c] .. src_ptr[c + 1]) of column c, 0 elsewhere
hipError_t launch_geo_scatter(int n, int k, const int* src_ptr, const int* src, double* B, int ldb, hipStream_t st);
// out[c * ldo + v] = sum over v's corners (m_ptr / m_idx order) of A_f (W_fj . X_f), X_f = -grad u / |grad u| (0 where grad u == 0)
hipError_t launch_geo_divergence(int n, int k, const int* F, const double* W, const double* Af, const int* m_ptr, const int* m_idx,
                                 const double* U, int ldu, double* out, int ldo, hipStream_t st);
// mean[c] = the mean of phi over column c's sources (list order); D[c * ldd + i] = phi[c * ldp + i] - mean[c]
hipError_t launch_geo_shift(int n, int k, const int* src_ptr, const int* src, const double* phi, int ldp, double* mean, double* D, int ldd,
                            hipStream_t st);

// as-rigid-as-possible deformation (smg_arap_device.hip).  rowptr / col / w: the CSR of the rest pose's cotangent matrix (diagonal entries
// are skipped); P0, P: rest and current positions as xyz rows; S, R: 9 doubles per vertex, row-major; B, U: column-major n x 3 ----------
// S_i = sum_j w_ij e_ij e'_ij^T in the row's stored order
hipError_t launch_arap_covariance(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, double* S, hipStream_t st);
// R_i = the closest rotation of S_i (smg_arap_inl.hpp), eterm[i] = sum_j w_ij |e'_ij - R_i e_ij|^2
hipError_t launch_arap_rotations(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, double* R, double* eterm,
                                 hipStream_t st);
// eterm[i] with the given rotations
hipError_t launch_arap_vertex_energy(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* R,
                                     double* eterm, hipStream_t st);
// B[c * ldb + i] = (sum_j (w_ij / 2) (R_i + R_j) e_ij)_c
hipError_t launch_arap_rhs(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* R, double* B, int ldb, hipStream_t st);
// P = U and U = P between xyz rows and a column-major block; the handle rows of U from hp (nh x 3 column-major, leading dimension ldh)
hipError_t launch_arap_rows(int n, const double* U, int ldu, double* P, hipStream_t st);
hipError_t launch_arap_columns(int n, const double* P, double* U, int ldu, hipStream_t st);
hipError_t launch_arap_set_handles(int nh, const int* handles, const double* hp, int ldh, double* U, int ldu, hipStream_t st);

// the fixed-order sum (smg_fixed_sum_device.hip): *sum = sum_i term[i] by fixed row chunks (part: fixed_sum_groups(n) doubles of scratch) and a
// fixed-order finalize; the bits depend on n and the terms alone ---------------------------------------------------------------------------
int fixed_sum_groups(int n);
hipError_t launch_fixed_sum(const double* term, int n, double* part, double* sum, hipStream_t st);
// *out = max_i term[i] through the same chunks and the same tree
hipError_t launch_fixed_max(const double* term, int n, double* part, double* out, hipStream_t st);

// disk parameterization (smg_param_device.hip).  UV, B: column-major nV x 2; per-face arrays are face-major planes (plane e at [e * nF + f]):
// rest (6: a, b, c, c0, c1, c2 of smg_param_inl.hpp), R (2: cos, sin), S (4); m_ptr / m_idx: the corner lists t = 3 f + i of every vertex,
// faces ascending; V0: nV x 3 row-major -------------------------------------------------------------------------------------------------
hipError_t launch_param_rest(int nF, const int* F, const double* V0, double* rest, hipStream_t st);
// S_f = sum_i c_i (u_i - u_{i+1}) (x_i - x_{i+1})^T
hipError_t launch_param_covariance(int nF, const int* F, const double* rest, const double* UV, int ld, double* S, hipStream_t st);
// R_f = the rotation closest to S_f, eterm[f] = (1/2) sum_i c_i |(u_i - u_{i+1}) - R_f (x_i - x_{i+1})|^2
hipError_t launch_param_local(int nF, const int* F, const double* rest, const double* UV, int ld, double* R, double* eterm, hipStream_t st);
// eterm[f] with the given rotations
hipError_t launch_param_face_energy(int nF, const int* F, const double* rest, const double* UV, int ld, const double* R, double* eterm, hipStream_t st);
// B[c * ldb + v] = (sum over v's corners of (1/2) R_f (c_i (x_i - x_{i+1}) + c_{i-1} (x_i - x_{i-1})))_c
hipError_t launch_param_rhs(int nV, int nF, const int* m_ptr, const int* m_idx, const double* rest, const double* R, double* B, int ldb, hipStream_t st);
// per face det J, sigma1, sigma2: out3 (3 planes), sigma (2 planes) and the 7 planes of terms the statistics reduce; each may be nullptr
hipError_t launch_param_distortion(int nF, const int* F, const double* rest, const double* UV, int ld, double* out3, double* sigma, double* terms,
                                   hipStream_t st);

// neo-Hookean membrane time step (smg_membrane_device.hip).  Vectors over the vertices are xyz rows (entry 3 v + l); per-face arrays are
// face-major planes (plane e at [e * nF + f]); m_ptr / m_idx: the corner lists t = 3 f + j of every vertex, faces ascending -----------------
// rest (5 planes): (abar^-1)00, 01, 11, det abar, thickness sqrt(det abar) / 4
hipError_t launch_membrane_rest(int nF, const int* F, const double* V0, double thickness, double* rest, hipStream_t st);
// mode 0: W (nF) alone; 1: W, G (9 planes), the upper triangle of the unfixed H (45 planes); 2: the same with the eigenvalue fix (smg_membrane_inl.hpp)
hipError_t launch_membrane_faces(int mode, int nF, const int* F, const double* P, const double* rest, double alpha, double beta, double floor,
                                 double value, double* W, double* G, double* H, hipStream_t st);
// the same for a material: 0 neo-Hookean (launch_membrane_faces with rest), 1 StVK, 2 tension-field StVK (k_membrane_faces_mat, which reads
// the rest pose V0 instead of rest); any other material is hipErrorInvalidValue
hipError_t launch_membrane_faces_material(int material, int mode, int nF, const int* F, const double* P, const double* V0, const double* rest,
                                          double thickness, double alpha, double beta, double floor, double value, double* W, double* G, double* H,
                                          hipStream_t st);
// val = M + dt2 K in the scalar CSR of the pattern (adjacency + I) (x) 1_3x3: block q of block row brow[q] (bptr: block rows, bcol: block
// columns) sums the face sub-blocks c_src[c_ptr[q] .. c_ptr[q + 1]) = 9 f + 3 a + b in list order; M = mass_scale mass0 on the diagonal
hipError_t launch_membrane_matrix(int nB, const int* brow, const int* bcol, const int* bptr, const int* c_ptr, const int* c_src, const double* H,
                                  int nF, double dt2, const double* mass0, double mass_scale, double* val, hipStream_t st);
// Qn (6 planes of scratch): e1 x e2 and the corners' shares of the mixed Voronoi area; mass[v] (optional) their sum over the vertex's corners;
// fext (optional) = (-(pressure mass_v)) (N / |N|), N the sum of e1 x e2 over the corners
hipError_t launch_membrane_pressure(int nV, int nF, const int* F, const double* P, const int* m_ptr, const int* m_idx, double pressure, double* Qn,
                                    double* mass, double* fext, hipStream_t st);
// g (optional) = the corner sums of G; b = -((M (qdot - qdot0) + dt g) + dt fext)
hipError_t launch_membrane_gradient(int nV, const int* m_ptr, const int* m_idx, const double* G, int nF, const double* mass0, double mass_scale,
                                    double dt, const double* qdot, const double* qdot0, const double* fext, double* g, double* b, hipStream_t st);
// t_out = qdot + step dx (dx == nullptr: qdot), p_out = pos0 + dt t_out, term[v] = p_v . fext_v + (M_v |t_v - qdot0_v|^2) / 2
hipError_t launch_membrane_trial(int nV, const double* qdot, const double* dx, double step, const double* qdot0, const double* pos0,
                                 const double* fext, const double* mass0, double mass_scale, double dt, double* t_out, double* p_out, double* term,
                                 hipStream_t st);
// term[v] = a_v . b_v
hipError_t launch_membrane_dot3(int nV, const double* a, const double* b, double* term, hipStream_t st);

// projective-dynamics membrane step (smg_pd_device.hip; the maths in smg_pd_inl.hpp).  x, vel, fext, V0: xyz rows (entry 3 v + l); S, Q, B:
// column-major nV x 3; per-face arrays are face-major planes (plane e at [e * nF + f]): rest (4: a, b, c, A_f), share (9: 3 i + l), Fg and T (6),
// sigma (2); m_ptr / m_idx: the corner lists t = 3 f + i of every vertex, faces ascending ------------------------------------------------
hipError_t launch_pd_rest(int nF, const int* F, const double* V0, double* rest, hipStream_t st);
// per face of the pose Q (coordinate l of vertex v at Q[v * sv + l * sl]): eterm[f] = (k A_f / 2) |F - T|_F^2 and share = k A_f (T g_i); Fg, sigma, T:
// all three or none (nullptr): the planes of the deformation gradient, its singular values and its projection onto the band [smin, smax]
hipError_t launch_pd_faces(int nF, const int* F, const double* rest, const double* Q, size_t sv, size_t sl, double k, double smin, double smax,
                           double* eterm, double* share, double* Fg, double* sigma, double* T, hipStream_t st);
// terms (5 planes): sigma1, -sigma2, outside the band (0 / 1), A_f |F - T|_F^2, A_f
hipError_t launch_pd_strain_terms(int nF, const double* rest, const double* Fg, const double* sigma, const double* T, double smin, double smax,
                                  double* terms, hipStream_t st);
// S_v = (x_v + h vel_v) + (h^2 (-fext_v + (rho m0_v) g)) / (rho m0_v); g: 3 doubles on the host
hipError_t launch_pd_predict(int nV, const double* x, const double* vel, const double* fext, const double* m0, double h, double rho, const double* g,
                             double* S, int ld, hipStream_t st);
// B_v = (c_mass m0_v) S_v + the corner shares of v in list order, iterm[v] = (c_mass m0_v / 2) |Q_v - S_v|^2, bsq[v] = |B_v|^2
hipError_t launch_pd_vertices(int nV, int nF, const int* m_ptr, const int* m_idx, const double* share, const double* m0, double c_mass, const double* S,
                              const double* Q, int ld, double* B, int ldb, double* iterm, double* bsq, hipStream_t st);
// vel = (Q - x) / h, x = Q
hipError_t launch_pd_finish(int nV, const double* Q, int ld, double h, double* x, double* vel, hipStream_t st);

// cubic and normal-driven stylization (smg_stylize_device.hip; the maths in smg_stylize_inl.hpp).  The CSR, P0, P and R as for smg_arap; nrm, tgt: xyz
// rows; area, lam (nullptr: the uniform p.lambda): one double per vertex; state: 7 planes of n (z, u, rho); iters: the ADMM iterations used -------
struct StyParams;
struct StyFrame;
// n_i, a_i from the corner lists t = 3 f + i of every vertex (mp, mi), faces ascending
hipError_t launch_stylize_normals(int n, const int* F, const int* mp, const int* mi, const double* V, double* nrm, double* area, hipStream_t st);
// the cubic local step (k_stylize_local): at most p.admm_iters ADMM iterations per vertex from state (fresh != 0: from z = u = 0, rho = p.rho0), the
// rotations, the state, eterm[i] = (1/2) sum_j w_ij |e'_ij - R_i e_ij|^2 + lambda_i a_i |Q R_i n_i|_1 and the iteration counts
hipError_t launch_stylize_cubic(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                const double* area, const double* lam, const StyFrame& Q, const StyParams& p, int fresh, double* state, double* R,
                                double* eterm, int* iters, hipStream_t st);
// the normal-driven local step: R_i = the closest rotation of S_i + 2 lambda_i a_i n_i t_i^T, eterm[i] with lambda_i a_i |R_i n_i - t_i|^2, iters[i] = 0
hipError_t launch_stylize_targets(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                  const double* area, const double* lam, const double* tgt, const StyParams& p, double* R, double* eterm, int* iters,
                                  hipStream_t st);
// eterm[i] with the given rotations (tgt != nullptr: the normal-driven term)
hipError_t launch_stylize_energy(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                 const double* area, const double* lam, const StyFrame& Q, const double* tgt, const StyParams& p, const double* R,
                                 double* eterm, hipStream_t st);

// feature-preserving denoising (smg_denoise_device.hip; the maths in smg_denoise_inl.hpp).  V0: xyz rows; per-face arrays are face-major planes
// (plane e at [e * nF + f]): rest (10: n, A, c, w), a normal field (3), share (9: 3 i + l); nb_ptr / nb_idx: N(f), the faces that share a vertex
// with f, ascending.  The right-hand side of the global step is launch_pd_vertices' (S = the input positions, c_mass = fidelity) -------------
hipError_t launch_denoise_rest(int nF, const int* F, const double* V0, double* rest, hipStream_t st);
// term[f] = sum over N(f), in list order, of |c_f - c_g|
hipError_t launch_denoise_spacing(int nF, const int* nb_ptr, const int* nb_idx, const double* rest, double* term, hipStream_t st);
// one iteration of the bilateral normal filter: m_out (another buffer than m_in) from m_in
hipError_t launch_denoise_filter(int nF, const int* nb_ptr, const int* nb_idx, const double* rest, const double* m_in, double sigma_s, double sigma_r,
                                 double* m_out, hipStream_t st);
// per face of the pose X (coordinate l of vertex v at X[v * sv + l * sl]) against the normals m: eterm[f] = (1/2) sum_k w_k h_k^2 and the corner shares
hipError_t launch_denoise_project(int nF, const int* F, const double* rest, const double* m, const double* X, size_t sv, size_t sl, double* eterm,
                                  double* share, hipStream_t st);

// gradient-domain morphing (smg_morph_device.hip; the maths in smg_morph_inl.hpp).  Poses are xyz rows; per-face arrays are face rows: W (9), nrm
// (3), omega (3), S (6: 00, 01, 02, 11, 12, 22), J and R (9); set c of J at c * 9 nF; B, U, hp: column-major, column 3c + d = coordinate d of set
// c; m_ptr / m_idx: the corner lists t = 3 f + i of every vertex, faces ascending ---------------------------------------------------------------
// W as launch_geo_basis, nrm = the unit normal, Af = A
hipError_t launch_morph_basis(const double* V, const int* F, int nF, double* W, double* nrm, double* Af, hipStream_t st);
// J[c][f] = T + N n^T of pose c (X + c * set_stride) on the rest face f of (S0, Fs); the rest basis is formed inside
hipError_t launch_morph_face_gradient(int nF, int k, const int* Fs, const double* S0, const double* X, size_t set_stride, double* J, hipStream_t st);
// the polar factors J = R S of the pose's gradients on the stored basis and omega = log R; R may be nullptr
hipError_t launch_morph_face_polar(int nF, const int* F, const double* W, const double* nrm, const double* X, double* R, double* omega, double* S,
                                   hipStream_t st);
// b_v = sum over v's corners (f, j), in list order, of A_f J_f W_fj; bsq[c * n + v] = |b_v|^2.  J_f is read, or recomputed from omega_f, S_f and t[c]
hipError_t launch_morph_rhs_gradient(int n, int k, int nF, const int* m_ptr, const int* m_idx, const double* W, const double* Af, const double* J,
                                     double* B, int ldb, double* bsq, hipStream_t st);
hipError_t launch_morph_rhs_interp(int n, int k, int nF, const int* m_ptr, const int* m_idx, const double* W, const double* Af, const double* omega,
                                   const double* S, const double* t, double* B, int ldb, double* bsq, hipStream_t st);
// U = the rest pose V in every set, or with X the blend (1 - t_c) V + t_c X; hp = the same at the pins; the pinned rows of U from hp
hipError_t launch_morph_start(int n, int k, const double* V, const double* X, const double* t, double* U, int ldu, hipStream_t st);
hipError_t launch_morph_pins(int nh, int k, const int* pins, const double* V, const double* X, const double* t, double* hp, int ldh, hipStream_t st);
hipError_t launch_morph_set_pins(int nh, int ncols, const int* pins, const double* hp, int ldh, double* U, int ldu, hipStream_t st);

// conformalized mean-curvature flow (smg_flow_device.hip; the maths in smg_flow_inl.hpp).  Positions are column-major nV x 3 blocks; m_ptr / m_idx:
// the corner lists t = 3 f + i of every vertex, faces ascending; part: fixed_sum_groups(max(nF, nV)) doubles; s: the block of FLOW_SUMS sums
// ([0] sphericity, [1] sum a, [2..4] sum a U, [5] sum a r, [6] sum a (r - rbar)^2, [8..11] the normalisation's, [12..15] the sphere map's) ---------
constexpr int FLOW_SUMS = 16;
// mass = the barycentric masses of U, B = mass U, val[j] = (-delta) L0[j] with the mass added at diag[row]: the values of M_t - delta L_0.
// mass_in (nullptr ok): the masses of this U where launch_flow_sphericity has just formed them (its `a`); they are then read, not gathered again
hipError_t launch_flow_system(int n, const double* U, int ldu, const int* F, const int* m_ptr, const int* m_idx, const int* rowptr, const int* diag,
                              const double* L0, double delta, const double* mass_in, double* mass, double* B, int ldb, double* val, hipStream_t st);
// out = U / sqrt(sum of double areas / 2), then x, y minus their means and z minus its minimum (normalize_unit_area); term: max(nF, n) doubles
hipError_t launch_flow_normalize(int n, int nF, const int* F, const double* U, int ldu, double* term, double* part, double* s, double* out, int ldo,
                                 hipStream_t st);
// s[0..6] of U; a, r: n doubles each, term: 3 n
hipError_t launch_flow_sphericity(int n, const double* U, int ldu, const int* F, const int* m_ptr, const int* m_idx, double* a, double* r, double* term,
                                  double* part, double* s, hipStream_t st);
// S = (U - c) / r with c from s_in[1..4]; sigma (2 planes of nF) rest face -> sphere face; terms (4 planes of nF) and their reductions
// s_out[0..3] = sum A sigma1 / sigma2, sum A, max sigma1 / sigma2, the flipped count
hipError_t launch_flow_sphere(int n, int nF, const int* F, const double* U, int ldu, const double* V0, int ld0, const double* s_in, double* S, int lds,
                              double* sigma, double* terms, double* part, double* s_out, hipStream_t st);

// Helmholtz-Hodge decomposition (smg_hodge_device.hip; the maths in smg_hodge_inl.hpp).  V: xyz rows; W, nrm, Af: 9, 3, 1 doubles per face; a field
// is nF x 3 row-major, set c at c * 3 nF; m_ptr / m_idx: the corner lists t = 3 f + i of every vertex, faces ascending ---------------------------
hipError_t launch_hodge_geometry(const double* V, const int* F, int nF, double* W, double* nrm, double* Af, hipStream_t st);
// Bb[c * ldb + v] = (1/2) sum (n_f x e_fi) . X_f, Bc[c * ldb + v] = -(1/2) sum e_fi . X_f over v's corners; bsq: 2 planes of k n, their squares
hipError_t launch_hodge_rhs(int n, int k, int nF, const int* m_ptr, const int* m_idx, const int* F, const double* V, const double* nrm, const double* X,
                            double* Bb, double* Bc, int ldb, double* bsq, hipStream_t st);
// parts (nullptr ok): G, R, H per face, set c at c * 9 nF; terms: plane 4 c + e of nF doubles = A_f |.|^2 of Xt, G, R, H
hipError_t launch_hodge_parts(int nF, int k, const int* F, const double* W, const double* nrm, const double* Af, const double* X, const double* u, int ldu,
                              const double* v, int ldv, double* parts, double* terms, hipStream_t st);
// X = grad u + n x grad v
hipError_t launch_hodge_field(int nF, int k, const int* F, const double* W, const double* nrm, const double* u, int ldu, const double* v, int ldv,
                              double* X, hipStream_t st);

// discrete conformal metrics (smg_conformal_device.hip; the maths in smg_conformal_inl.hpp).  u, s, sum, g: nV; ang, hc, l0, lt: nF x 3 in corner
// order (3 f + c); area2: nF, twice the rest area; broken: nF doubles, 1.0 / 0.0; m_ptr / m_idx: the corner lists; (rowptr; l_ptr, l_idx, l_sgn): the CSR's rows and the assembly
// recipe of its entries (AssemblyPlan) ---------------------------------------------------------------------------------------------------------------
// ut = u + t d (d == nullptr: u), s = exp(-ut / 2)
hipError_t launch_conformal_scale(int n, const double* u, const double* d, double t, double* ut, double* s, hipStream_t st);
hipError_t launch_conformal_faces(int nF, const int* F, const double* l0, const double* area2, const double* s, double* ang, double* hc, double* broken,
                                  hipStream_t st);
hipError_t launch_conformal_lengths(int nF, const int* F, const double* l0, const double* s, double* lt, hipStream_t st);
// sum = the angle sums, g = sum - Theta (0 where fixed[v] != 0), gsq = g^2, gabs = |g|; val (nullptr ok) = the values of -L~; red (nullptr ok) =
// sum g^2, max |g|, the broken count (part: fixed_sum_groups(max(n, nF)) doubles)
hipError_t launch_conformal_rows(int n, int nF, const double* ang, const double* hc, const double* broken, const int* m_ptr, const int* m_idx,
                                 const double* Theta, const int* fixed, const int* rowptr, const int* l_ptr, const int* l_idx, const signed char* l_sgn,
                                 double* sum, double* g, double* gsq, double* gabs, double* val, double* part, double* red, hipStream_t st);
// u[list[i]] = values[i] (values == nullptr: 0)
hipError_t launch_conformal_fix(int nf, const int* list, const double* values, double* u, hipStream_t st);

// earth mover's distance (smg_emd_device.hip; the maths in smg_emd_inl.hpp).  V: xyz rows; W2, Af: 6, 1 doubles per face; the state ZU: 4 doubles per
// (face, column), Z then U, column c at c * 4 nF; a field in the faces' frames: 2 doubles per (face, column); rho, gmax2: k doubles on the device;
// m_ptr / m_idx: the corner lists t = 3 f + i of every vertex, faces ascending --------------------------------------------------------------------
hipError_t launch_emd_geometry(const double* V, const int* F, int nF, double* W2, double* Af, hipStream_t st);
// R[c * ldr + v] = sum A_f (W2_fi . X_f) over v's corners - b[c * ldb + v]; state: X is ZU and X_f = Z_f - U_f, else a field in the frames;
// dsq (nullptr ok): k planes of n, the squares with vertex 0's zero
hipError_t launch_emd_rhs(int n, int k, int nF, const int* m_ptr, const int* m_idx, const double* W2, const double* Af, const double* X, bool state,
                          const double* b, int ldb, double* R, int ldr, double* dsq, hipStream_t st);
// one ADMM update of ZU in place from phi; J2 (nullptr ok): J in the frames; up, gq: k planes of nF, A_f |J_f| and rho^2 |grad phi_f|^2
hipError_t launch_emd_update(int nF, int k, const int* F, const double* W2, const double* Af, const double* phi, int ldp, double* ZU, const double* rho,
                             double alpha, double* J2, double* up, double* gq, hipStream_t st);
// pot = (-rho / max(1, sqrt(gmax2))) phi; terms: k planes of n, b pot
hipError_t launch_emd_dual(int n, int k, const double* b, int ldb, const double* phi, int ldp, const double* rho, const double* gmax2, double* pot, int ldq,
                           double* terms, hipStream_t st);
// out (3 doubles per (face, column)) = J2[0] t1 + J2[1] t2
hipError_t launch_emd_flow(int nF, int k, const double* V, const int* F, const double* J2, double* out, hipStream_t st);

// incompressible flow on a surface, vorticity form (smg_fluid_device.hip; the maths in smg_fluid_inl.hpp).  W, nrm, Af: launch_hodge_geometry's; m:
// the barycentric masses; known: 1 on the rows whose psi is given; dt, mwsum, rmax: k doubles per row on the device; per-vertex term planes are k
// planes of n; m_ptr / m_idx: the corner lists t = 3 f + i of every vertex, faces ascending -----------------------------------------------------
hipError_t launch_fluid_mass(int n, const int* m_ptr, const int* m_idx, const double* Af, double* m, hipStream_t st);
// R[c * ldr + v] = 0.0 - m_v (w - wbar_c), wbar_c = mwsum[c] / *msum (mwsum nullptr: 0.0); rsq: the squares, 0.0 on the known rows
hipError_t launch_fluid_rhs(int n, int k, const double* m, const int* known, const double* w, int ldw, const double* mwsum, const double* msum, double* R,
                            int ldr, double* rsq, hipStream_t st);
// one stage: out = a wn + b (w + dt_c adv(psi, w)), rate = the outflow over m, mw = m out; rates_only: rate alone (w, wn, dt, out, mw unread).
// out must not be w (refused)
hipError_t launch_fluid_advect(int n, int k, const int* F, const int* m_ptr, const int* m_idx, const double* m, const double* psi, int ldp,
                               const double* w, int ldw, const double* wn, int ldn, double a, double b, const double* dt, double theta, double* out,
                               int ldo, double* rate, double* mw, bool rates_only, hipStream_t st);
// op 0: dt[c] = cfl / rmax[c] (0.0 where rmax is not > 0); op 1: his_cfl[c] = dt[c] max_s rmax[s * k + c], time[c] += dt[c], his_time[c] = time[c]
hipError_t launch_fluid_dt(int op, int k, int stages, double cfl, const double* rmax, double* dt, double* time, double* his_cfl, double* his_time,
                           hipStream_t st);
// U (nullptr ok; 3 doubles per (face, column)) = n x grad psi; terms: k planes of nF, 0.5 (A_f |grad psi_f|^2)
hipError_t launch_fluid_velocity(int nF, int k, const int* F, const double* W, const double* nrm, const double* Af, const double* psi, int ldp, double* U,
                                 double* terms, hipStream_t st);
// mw = m w, ew (nullptr ok) = 0.5 ((m w) w): k planes of n each
hipError_t launch_fluid_diag(int n, int k, const double* m, const double* w, int ldw, double* mw, double* ew, hipStream_t st);

// two-species reaction-diffusion on a surface (smg_rd_device.hip; the maths in smg_rd_inl.hpp).  m: the barycentric masses of launch_fluid_mass;
// u, v and the outputs: column-major blocks of k columns with a leading dimension; coef: k x 20 on the device; per-vertex term planes are planes
// of n.  One wavefront per (64 vertices, column) ----------------------------------------------------------------------------------------------
// (u, v) through `substeps` Euler steps of length h of the column's cubic reaction; Ru = m u*, Rv = m v*; rsq: 2k planes, the squares of Ru then
// of Rv; vout (nullptr ok) = v*
hipError_t launch_rd_react(int n, int k, const double* m, const double* u, const double* v, int ld, const double* coef, double h, int substeps,
                           double* Ru, double* Rv, int ldr, double* rsq, double* vout, int ldv, hipStream_t st);
// mt: 2k planes, m u1 then m v1; chg: k planes, max(|u1 - u0|, |v1 - v0|)
hipError_t launch_rd_close(int n, int k, const double* m, const double* u0, const double* v0, const double* u1, const double* v1, int ld, double* mt,
                           double* chg, hipStream_t st);

// the wave equation on a surface (smg_wave_device.hip; the maths in smg_wave_inl.hpp).  mt = m / speed^2, s2 = 2.0 + sigma dt: planes of n; known
// (nullptr ok): 1 on the clamped rows; u, v, b, z, w: column-major blocks of k columns with a leading dimension; per-vertex term planes are k planes
// of n.  One wavefront per (64 vertices, column); the list kernels one lane per (entry, column) --------------------------------------------------
// b = mt (s2 u + dt v), z = 2 u + dt v (both with leading dimension ldb), rsq = b^2 (0.0 on the known rows)
hipError_t launch_wave_rhs(int n, int k, const double* mt, const double* s2, const int* known, double dt, const double* u, const double* v, int ld, double* b,
                           double* z, int ldb, double* rsq, hipStream_t st);
// b += a (sig0 + sig1) at the n_src vertices idx (no vertex twice), sig0 and sig1 n_src x k row-major; rsq rewritten there
hipError_t launch_wave_sources(int n, int k, int n_src, const int* idx, const double* sig0, const double* sig1, double a, double* b, int ldb, double* rsq,
                               hipStream_t st);
// un = w - u, vn = q2 (un - u) - v, ke = 0.5 ((mt vn) vn); bnext != nullptr: launch_wave_rhs of (un, vn) into bnext, znext, rsqnext as well; znext may
// be w (with ldb == ldw): the warm start then replaces the answer it was formed from
hipError_t launch_wave_advance(int n, int k, const double* mt, const double* s2, const int* known, double dt, double q2, const double* w, int ldw,
                               const double* u, const double* v, int ld, double* un, double* vn, int ldn, double* ke, double* bnext, double* znext, int ldb,
                               double* rsqnext, hipStream_t st);
// out (n_rec x k row-major) = u at the vertices idx
hipError_t launch_wave_record(int n, int k, int n_rec, const int* idx, const double* u, int ld, double* out, hipStream_t st);
// flag (n_rows x k) = 1.0 where u or v is not 0.0 on a listed row, else 0.0
hipError_t launch_wave_rows_nonzero(int n, int k, int n_rows, const int* rows, const double* u, const double* v, int ld, double* flag, hipStream_t st);

// the wave object's adjoint pass (smg_wave_adjoint_device.hip; the maths in smg_wave_adjoint_inl.hpp).  p, q, y, G: column-major blocks of k columns
// with a leading dimension; a history block e and the squares are k planes of n; a trace row is (receiver slot) x column ------------------------------
// e = dt v - (0.5 s2) (u1 - u): what the adjoint pass reads of a forward step from (u, v) to u1
hipError_t launch_wave_adj_keep(int n, int k, const double* s2, double dt, const double* u, const double* v, const double* u1, int ld, double* e, hipStream_t st);
// rho = trace - observed (nullptr: zeros) over `entries` (rows x slots) x k values, sq: their squares in k planes of `entries`
hipError_t launch_wave_adj_residual(int k, long long entries, const double* trace, const double* observed, double* rho, double* sq, hipStream_t st);
// p += R' rho for one trace row: group j is the vertex grp_v[j] with the slots grp_slot[grp_ptr[j] .. grp_ptr[j + 1]), added in that order
hipError_t launch_wave_adj_inject(int n, int k, int n_grp, const int* grp_v, const int* grp_ptr, const int* grp_slot, const double* rho, double* p, int ld,
                                  hipStream_t st);
// g = p + q2 q (leading dimension ldg), gsq = g^2, both 0.0 on the known rows
hipError_t launch_wave_adj_rhs(int n, int k, const int* known, double q2, const double* p, const double* q, int ld, double* g, int ldg, double* gsq,
                               hipStream_t st);
// G += y e, t = mt y, p = (s2 t - p) - (2.0 q2) q, q = dt t - q, in place
hipError_t launch_wave_adj_advance(int n, int k, const double* mt, const double* s2, double dt, double q2, const double* y, int ldy, const double* e, double* p,
                                   double* q, double* G, int ld, hipStream_t st);
// gs0 += a y, gs1 += a y at the n_src vertices idx (no vertex twice); gs0, gs1 n_src x k row-major
hipError_t launch_wave_adj_signal(int n, int k, int n_src, const int* idx, double a, const double* y, int ld, double* gs0, double* gs1, hipStream_t st);
// out = fac G; out may be G
hipError_t launch_wave_adj_scale(int n, int k, const double* fac, const double* G, int ld, double* out, int ldo, hipStream_t st);

// the distributed source of a tangent (Born) step (smg_wave_born_device.hip; the maths in smg_wave_born_inl.hpp): off the known rows
// b = b + fd[i, c % d_cols] e[i, c] and rsq = b^2; fd: d_cols planes of n, e: k planes of n, b: column-major with leading dimension ldb
hipError_t launch_wave_born(int n, int k, int d_cols, const int* known, const double* fd, const double* e, double* b, int ldb, double* rsq, hipStream_t st);

}  // namespace smg
