// smg_mesh_object.hpp -- what an object built on a triangle mesh and a caller's hierarchy starts from (smg_geodesics.cpp, smg_arap.cpp,
// smg_membrane.cpp, smg_param.cpp): the checks of a create call, the object's stream, device and cloned handles, the cotangent system
// assembled on the device, the inner solve and its default options, the copies of a call's blocks, and the byte total.  `who` is the entry
// point's name, the prefix of every message.  The local / global loop of smg_arap_solve and smg_param_arap: smg_local_global.hpp.
#pragma once
#include <vector>

#include "smg_internal.hpp"

namespace smg {

double double_area(const double* V, const int* F, int f);   // twice the area of face f, the expression of k_face_terms / k_geo_basis
int components(const int* F, int nF, int nV);               // connected components of the vertex graph (a vertex in no face is one)
int level0_rows(const smg_hierarchy* h);                    // rows of level 0 of a hierarchy whose prolongations are set (-1: none set)
int copy_prolongations(const smg_hierarchy* src, smg_hierarchy* dst);
long long handle_bytes(const smg_hierarchy* h);             // the sum of device_byte_entries (nullptr: 0)

// ---- the checks of a create call, in this order; none of them touches the device ------------------------------------------------------------
// h is no union handle, has `dofs` (1 or 3) unknowns per vertex, and dofs * nV rows on level 0
int check_hierarchy(const char* who, const smg_hierarchy* h, int dofs, int nV);
int check_faces(const char* who, const int* F, int nF, int nV);   // every index in [0, nV)
// check_faces, every double area > 0 (*area2, optional: their sum), every coordinate finite, and with `connected` one component
int check_mesh(const char* who, const double* V, int nV, const int* F, int nF, bool connected, double* area2 = nullptr);

// ---- the object's stream, device and handles.  The object derives from this and declares its buffers as DevBuf members; its destructor is
// { quiesce(); }, so that teardown runs: stream synchronised, handles destroyed (quiesce), buffers freed (the members), stream destroyed (here).
struct MeshObject {
    hipStream_t stream = nullptr;
    int device = -1;
    smg_hierarchy* handle[2] = {nullptr, nullptr};                    // smg_geodesics and smg_hodge (a mesh with boundary) hold two; smg_conformal one
    MeshObject() = default;
    MeshObject(const MeshObject&) = delete;
    MeshObject& operator=(const MeshObject&) = delete;
    int open(const char* who);                                        // a HIP device exists (SMG_ERR_NO_DEVICE); the current device, a stream of its own
    int clone(const char* who, const smg_hierarchy* src, int slot);   // handle[slot] = src's levels and prolongations, on the object's stream
    void quiesce();
    ~MeshObject() { if (stream) (void)hipStreamDestroy(stream); }
};

// the object's share of HBM: its handles and every buffer of the one list the object passes
template <class... Bufs>
long long device_bytes(const MeshObject& o, const Bufs&... bufs) { return ((handle_bytes(o.handle[0]) + handle_bytes(o.handle[1])) + ... + bufs.bytes()); }

// ---- smg_assemble on d_V (nV x 3 row-major, device) back on the host as CSR: the pattern, L's values, and with `val` c_mass M + c_L L
// (voronoi: the mass type).  keep_L (optional) keeps L's values on the device.  Synchronises the stream.
struct CotanSystem { std::vector<int> ptr, col; std::vector<double> L, val; };
int cotan_system(const int* F, int nF, int nV, const double* d_V, int voronoi, double c_mass, double c_L, hipStream_t st, CotanSystem& S, bool val,
                 DevBuf<double>* keep_L = nullptr);

// ---- the inner solver of an object: smg_solve_pcg (pcg != 0) or smg_solve on device blocks; *entries (optional) = the loop entries of a
// solve that returned SMG_OK.  latch_solver: the rule of the set_solver calls, -1 keeps, else 0 / 1.
int inner_solve(smg_hierarchy* h, int pcg, const double* B, int ldb, const double* known, int ld_kv, const double* z0, int ld_z0, int k,
                const smg_solve_opts& o, double* z, int ld_z, int* entries);
inline void latch_solver(int& pcg, int v) { if (v >= 0) pcg = v ? 1 : 0; }
// the caller's options, or smg_solve_opts_default with this tol and (max_iter > 0) this max_iter
smg_solve_opts opts_or_default(const smg_solve_opts* opts, double tol, int max_iter = 0);

// ---- the blocks a call moves: the memspace argument and its two copy kinds; rows x k doubles between column-major blocks with leading
// dimensions ld_dst, ld_src; F (nF x 3) and the corner lists t = 3 f + i of every vertex, faces ascending, onto the device (mp, mi: kept on the host too)
inline bool bad_memspace(int memspace) { return memspace != SMG_HOST && memspace != SMG_DEVICE; }
inline hipMemcpyKind copy_in(int memspace) { return memspace == SMG_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice; }
inline hipMemcpyKind copy_out(int memspace) { return memspace == SMG_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; }
inline hipError_t copy_columns(double* dst, int ld_dst, const double* src, int ld_src, int rows, int k, hipMemcpyKind kind, hipStream_t st)
{
    return hipMemcpy2DAsync(dst, (size_t)ld_dst * sizeof(double), src, (size_t)ld_src * sizeof(double), (size_t)rows * sizeof(double), (size_t)k, kind, st);
}
int upload_faces(const int* F, int nF, int nV, DevBuf<int>& d_F, DevBuf<int>& d_ptr, DevBuf<int>& d_idx, std::vector<int>* mp = nullptr,
                 std::vector<int>* mi = nullptr);

// ---- smg_stylize.cpp: what smg_stylize_local_host and smg_debug_stylize check alike, in this order (operands, parameters, faces, the CSR, then
// lambda, frame and targets where given), and the parameters as the kernels take them
struct StyParams;
StyParams sty_params(const smg_stylize_params& p);
int stylize_check_operands(const char* who, int op, int nV, int nF, const int* F, const int* rowptr, const int* col, const double* w, const double* V0,
                           const double* P, const double* lam, const double* Q, const double* targets, const double* R_in,
                           const smg_stylize_params* p, const double* out, const int* iters);

// ---- smg_morph.cpp: what smg_morph_faces_host and smg_debug_morph check alike, in this order: the op and its operands, k, the times, the faces,
// the pins
int morph_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V0, const double* X, const double* t,
                         const double* in, const int* pins, int n_pins, const double* out);

// ---- smg_flow.cpp: what smg_flow_host and smg_debug_flow check alike, in this order: the op and its operands, the faces, then for the system
// delta and the CSR (monotone row pointers, columns in range, one stored diagonal entry per row); the position of every row's diagonal entry
int flow_check_operands(const char* who, int op, int nV, int nF, const int* F, const double* U, const double* V0, const int* rowptr, const int* col,
                        const double* L0, double delta, const double* out);
void flow_diagonal(int nV, const int* rowptr, const int* col, std::vector<int>& diag);

// ---- smg_hodge.cpp: what smg_hodge_host and smg_debug_hodge check alike, in this order: the op and its operands, k, the faces
int hodge_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* X, const double* u, const double* v,
                         const double* out);

// ---- smg_conformal.cpp: what smg_conformal_host and smg_debug_conformal check alike, in this order: the op and its operands, the faces, a finite
// trial step, the fixed list (in range, no vertex twice; empty is allowed here)
int conformal_check_operands(const char* who, int op, int nV, int nF, const int* F, const double* l0, const double* area2, const double* u, const double* d, double t,
                             const double* s, const double* Theta, const int* fixed, int n_fixed, const double* out);

// ---- smg_emd.cpp: what smg_emd_host and smg_debug_emd check alike, in this order: the op and its operands, k, the faces
int emd_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* b, const double* phi, const double* state,
                       const double* rho, const double* out);

// ---- smg_fluid.cpp: what smg_fluid_host and smg_debug_fluid check alike, in this order: the op and its operands, k, theta (a full stage), the faces
int fluid_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* w, const double* psi, const double* wn,
                         const double* dt, double theta, int rates_only, const double* out);

// ---- smg_rd.cpp: what smg_rd_host and smg_debug_rd check alike, in this order: the op and its operands, k, then for the reaction the sub-steps,
// dt and the coefficients (finite), the faces
int rd_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* u, const double* v, const double* coeff,
                      double dt, int substeps, const double* un, const double* vn, const double* out);

// ---- smg_sinkhorn.cpp: what smg_sinkhorn_host checks, in this order: the op and its operands, k, then for the scale
// and the geomean k_in and the floor (finite and >= 0), the faces
int sinkhorn_check_operands(const char* who, int op, int nV, int nF, int k, int k_in, const int* F, const double* V, const double* y, const double* r,
                            const double* mu, const double* mu1, const double* sr, const double* alphas, double floor, const double* out);

// ---- smg_wave.cpp: what smg_wave_host and smg_debug_wave check alike, in this order: the op and its operands, k, dt, clamped, speed (finite and
// > 0), sigma (finite and >= 0), the faces, then the list of a source or record op: at least one vertex, in range, as sources no vertex twice
int wave_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma, int clamped,
                        double dt, const double* u, const double* v, const double* w, const int* idx, int n_idx, const double* sig0, const double* sig1,
                        const double* out);

}  // namespace smg
