// smg_wave_object.hpp -- the wave object's state and what its two translation units share (smg_wave.cpp: create, the state, the lists, the forward
// step; smg_wave_adjoint.cpp: smg_wave_gradient, smg_wave_set_speed; smg_wave_born.cpp: smg_wave_gauss_newton; include/smg.h: smg_wave_*; DESIGN.md
// sections 33, 34 and 36).
#pragma once
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

struct smg_wave : smg::MeshObject {        // handle[0]: diag(0.5 s2 mt) + a (-L), the boundary known when clamped
    int nV = 0, nF = 0, nb = 0;            // nb: the clamped rows (0: free boundary)
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    bool fused = true;                     // the advance kernel leaves the next step's right-hand side (SMG_WAVE_FUSED=0 at create: it does not)
    bool has_sigma = false, rhs_valid = false;
    smg_wave_params p;
    double a = 0.0, q2 = 0.0;              // 0.25 dt dt, 2.0 / dt
    size_t kcap = 0;                       // the columns the state's blocks hold
    int k = 0, cur = 0;                    // the state's columns (0: none); which of S[2] holds the state
    int n_src = 0, n_rec = 0;
    smg::CotanSystem Sys;                  // the pattern and -L's values
    std::vector<double> mt_host, sigma_host, red_host;
    std::vector<int> bnd, on_bnd;          // the clamped rows; 1 on them (empty: free)
    smg::DevBuf<int> F, known, rows, src, rec;  // faces; 1 on the clamped rows; the clamped rows; the source and receiver vertices
    smg::DevBuf<double> W, nrm, Af;        // gradient basis (9 per face), normals (3), areas: the potential energy's geometry
    smg::DevBuf<double> mt, s2, val;       // planes of n; the system's values on their way to the handle
    smg::DevBuf<double> S[2], B, Wb;       // column-major n x 2k: the state and the step's output; n x k: right-hand side; the warm start, then the solve's answer
    smg::DevBuf<double> rsq, ke, terms;    // k planes of n: squares, kinetic terms; k planes of nF: the potential terms
    smg::DevBuf<double> part, red;         // the chunk sums; |b|^2 then k kinetic and k potential energies
    smg::DevBuf<double> zero, flag;        // nb x k: the known rows' values; set_state's check of them
    smg::DevBuf<double> sig, trace;        // a call's signal and its traces
    // ---- smg_wave_gradient and smg_wave_set_speed (smg_wave_adjoint.cpp): nothing below is allocated before the first gradient call
    std::vector<double> m_host, speed_host;     // the masses; the speed (empty: 1 everywhere)
    std::vector<int> rec_host;             // the receiver list as given
    bool grouped = false, fac_valid = false;    // the grouped list matches rec_host; fac matches mt_host and speed_host
    int n_grp = 0;                         // the receivers' distinct vertices that are on no clamped row
    smg::DevBuf<int> grp_v, grp_ptr, grp_slot;  // per group its vertex; its slots grp_slot[grp_ptr[j] .. grp_ptr[j + 1]), ascending
    smg::DevBuf<double> H;                 // the history: n_steps blocks e_n of n x k
    smg::DevBuf<double> P, Q, Y, G;        // n x k each: the adjoint state, the adjoint solve's answer (the next one's warm start), sum_n y e_n
    smg::DevBuf<double> rho, apart, ared;  // the residuals, their squares (k planes) and the observed traces; the misfit's chunk sums; its k sums
    smg::DevBuf<double> gs, fac;           // the signal's gradient; the plane (-2 mt) / speed
    // ---- smg_wave_gauss_newton (smg_wave_born.cpp): nothing below is allocated before the first product call
    bool lin_valid = false;                // H holds the history of a completed gradient call with a backward pass: the linearisation point
    int lin_steps = 0;                     // its steps; its columns are k (a set_state that changes k drops the point)
    smg::DevBuf<double> T[2], fd;          // column-major n x 2k: the tangent state and the tangent step's output; n x d_cols: fac d
    ~smg_wave() { quiesce(); }
};

namespace smg {

// s2, a, q2 from p and the handle's values diag(0.5 s2 mt) + a (-L) from the kept pattern; first: the pattern-setting precompute with the
// clamped rows known, else by values.  Drops the kept right-hand side
int wave_system(smg_wave* g, bool first);
// the checks of a stepping call, in this order: the object and its state, n_steps >= 1; then the signal: sources are set, every entry finite
int wave_check_steps(const char* who, const smg_wave* g, int n_steps);
int wave_check_signal(const char* who, const smg_wave* g, int n_steps, const double* signal);
// the optional operands of a tangent (Born) run: fd = fac d (n x d_cols, d_cols 1 or k) and the kept history, n_steps blocks e_n of n x k
struct WaveBorn {
    const double* fd;
    int d_cols;
    const double* e;
};
// the steps of smg_wave_step after its checks, on the state blocks S[0], S[1] (n x 2k each) of which S[*cur] holds the state; a completed step
// flips *cur.  record: the traces are gathered on the device (g->trace) even where `traces` is nullptr; keep (device, nullptr ok): n_steps
// blocks of n x k, block t = dt v_t - (0.5 s2) (u_t+1 - u_t) of step t, one more launch per step.  born (nullptr: none): the tangent run --
// k_wave_born adds fd e_t to the right-hand side of step t, and a right-hand side that is exactly 0.0 skips the solve with w = 0 and a cycles
// entry of 0
int wave_forward(smg_wave* g, const char* who, smg::DevBuf<double>* S, int* cur, const WaveBorn* born, int n_steps, const double* signal,
                 const smg_solve_opts* opts, double* energy_his, double* traces, bool record, int* cycles, int* n_done, double* keep);

// ---- smg_wave_adjoint.cpp: what smg_wave_adjoint_host and smg_debug_wave_adjoint check alike, in this order: the op and its operands, k, dt, clamped,
// speed, sigma, the faces, then the rows and the list of a list op (sources: no vertex twice)
int wave_adjoint_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma,
                                int clamped, double dt, const double* x0, const double* x1, const double* x2, const double* x3, const double* x4, const int* idx,
                                int n_idx, int n_rows, const double* out);

// ---- smg_wave_adjoint.cpp, shared with smg_wave_born.cpp -----------------------------------------------------------------------------------------
// the blocks of a gradient call; they grow with the largest shape seen and are kept.  The receivers are grouped by vertex where the list has
// changed, the factor plane is formed where the speed has
int wave_ensure_adjoint(smg_wave* g, int n_steps, bool backward, bool observed, bool grad_signal);
// the backward loop of smg_wave_gradient from p = R' rho_N, q = 0, Y = 0, G = 0 over the kept history g->H: leaves (p, q) in g->P, g->Q, the
// unscaled sum_n y e_n in g->G and, where grad_signal, the signal's gradient in g->gs.  rho: the residuals on the device, n_steps rows of
// n_rec x k; cycles (nullptr ok): n_steps entries in the order the solves ran.  Drops the kept right-hand side
int wave_backward(smg_wave* g, const char* who, int n_steps, const double* rho, const smg_solve_opts* opts, bool grad_signal, int* cycles);

// ---- smg_wave_born.cpp: what smg_wave_born_host and smg_debug_wave_born check alike, in this order: the sizes, F and out; the operands; k; d_cols;
// clamped; the faces
int wave_born_check_operands(const char* who, int nV, int nF, int k, int d_cols, const int* F, int clamped, const double* b, const double* e,
                             const double* fd, const double* out);

}  // namespace smg
