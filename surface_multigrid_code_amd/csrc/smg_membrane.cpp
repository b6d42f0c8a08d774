// smg_membrane.cpp -- implicit-Euler steps of a pressurised membrane (neo-Hookean, StVK or tension-field StVK) on the block V-cycle (include/smg.h: smg_membrane_*;
// DESIGN.md section 20; the reference's 06_example_balloon_sim: main.cpp:109-134, implicit_euler_mg_balloon.h:35-121).
// The object owns one handle built from the caller's block prolongations and precomputed with H = M + dt^2 K of the rest pose, the mesh and
// its lists on the device (corner lists per vertex, contribution lists per 3 x 3 block), the rest constants per face, and the state
// (pos, qdot) with the buffers of a step.  A Newton iteration: per-face energy / gradient / fixed Hessian (k_membrane_faces), H in the
// caller-order CSR (k_membrane_matrix), b (k_membrane_gradient), the value-only re-precompute, one solve from zero, b . dx, and the
// backtracking line search, which per trial costs k_membrane_trial + the energy-only face kernel + the fixed-order reduction and one double
// read by the host.  All of it is enqueued on the object's stream, which the handle uses too.  Checks, stream, handle and the inner solve:
// smg_mesh_object.hpp; the lists and lame(): smg_membrane_inl.hpp; the objective's sum: launch_fixed_sum.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_membrane_inl.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

namespace smg {

// the pattern (adjacency + I) in block CSR with sorted columns, and per block the sub-blocks (corner a, corner b) of the faces that touch it
void membrane_lists(const int* F, int nF, int nV, MembraneLists& L)
{
    struct Item { int i, j, src; };
    std::vector<Item> items;
    items.reserve(9 * (size_t)nF);
    for (int f = 0; f < nF; f++)
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) items.push_back({F[3 * (size_t)f + a], F[3 * (size_t)f + b], 9 * f + 3 * a + b});
    std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) {
        return x.i != y.i ? x.i < y.i : x.j != y.j ? x.j < y.j : x.src < y.src;
    });
    L.bptr.assign((size_t)nV + 1, 0);
    L.bcol.clear(); L.brow.clear(); L.c_ptr.clear(); L.c_src.clear();
    for (size_t t = 0; t < items.size(); t++) {
        if (t == 0 || items[t].i != items[t - 1].i || items[t].j != items[t - 1].j) {
            L.brow.push_back(items[t].i);
            L.bcol.push_back(items[t].j);
            L.c_ptr.push_back((int)t);
            L.bptr[items[t].i + 1]++;
        }
        L.c_src.push_back(items[t].src);
    }
    L.c_ptr.push_back((int)items.size());
    for (int v = 0; v < nV; v++) L.bptr[v + 1] += L.bptr[v];
}

}  // namespace smg

struct smg_membrane : MeshObject {             // handle[0]: H = M + dt^2 K, block
    int nV = 0, nF = 0, nB = 0;
    int pcg = 0;                               // the inner solver: 0 smg_solve (the reference's loop), 1 smg_solve_pcg
    int material = 0;                          // 0 neo-Hookean, 1 StVK, 2 tension-field StVK (smg_membrane_set_material)
    smg_membrane_params p;
    double alpha = 0.0, beta = 0.0;            // the Lame parameters (main.cpp:63-67)
    DevBuf<int> F, m_ptr, m_idx, brow, bcol, bptr, c_ptr, c_src;
    DevBuf<double> V0, rest, mass0;            // rest positions, rest constants (5 planes), Voronoi mass of the rest pose
    DevBuf<double> pos, qdot, posT, qdotT, pos0, qdot0;   // the state, the line search's trial, the state at the start of the step
    DevBuf<double> fext, b, dx, zero, Hval;    // pressure force, right-hand side, Newton direction, the solve's start, H in the caller's CSR order
    DevBuf<double> G, H, Qn, terms, part, E;   // per-face planes (9, 45, 6), the objective's terms (nF + nV), their chunk sums, the reduced values
    ~smg_membrane() { quiesce(); }
};

namespace {

const char* bad_params(const smg_membrane_params& p)
{
    auto finite = [](double x) { return std::isfinite(x); };
    if (!finite(p.dt) || !(p.dt > 0.0)) return "dt must be > 0";
    if (!finite(p.poisson) || !(std::fabs(p.poisson) < 1.0)) return "|poisson| must be < 1";
    if (!finite(p.young) || !(p.young > 0.0)) return "young must be > 0";
    if (!finite(p.thickness) || !(p.thickness > 0.0)) return "thickness must be > 0";
    if (!finite(p.mass_scale) || !(p.mass_scale > 0.0)) return "mass_scale must be > 0";
    if (p.newton_iters < 0) return "newton_iters must be >= 0";
    if (!finite(p.eig_value) || !(p.eig_value > 0.0)) return "eig_value must be > 0";
    if (!finite(p.pressure) || !finite(p.eig_floor) || !finite(p.ls_c)) return "a parameter is not finite";
    if (!(p.ls_shrink > 0.0 && p.ls_shrink < 1.0) || !(p.ls_min_alpha > 0.0)) return "ls_shrink must lie in (0, 1) and ls_min_alpha be > 0";
    return nullptr;
}

// W, G, H' at P into the object's planes (W in terms[0 .. nF)), then H in the CSR order and b
int assemble(smg_membrane* m, const double* P, const double* qdot, const double* qdot0)
{
    const smg_membrane_params& p = m->p;
    hipStream_t st = m->stream;
    HIPCHK(launch_membrane_faces_material(m->material, 2, m->nF, m->F.p, P, m->V0.p, m->rest.p, p.thickness, m->alpha, m->beta, p.eig_floor,
                                          p.eig_value, m->terms.p, m->G.p, m->H.p, st));
    HIPCHK(launch_membrane_matrix(m->nB, m->brow.p, m->bcol.p, m->bptr.p, m->c_ptr.p, m->c_src.p, m->H.p, m->nF, p.dt * p.dt, m->mass0.p,
                                  p.mass_scale, m->Hval.p, st));
    HIPCHK(launch_membrane_gradient(m->nV, m->m_ptr.p, m->m_idx.p, m->G.p, m->nF, m->mass0.p, p.mass_scale, p.dt, qdot, qdot0, m->fext.p, nullptr,
                                    m->b.p, st));
    return SMG_OK;
}

// f(qdot + step dx) (dx == nullptr: f(qdot)); the trial state is left in qdotT / posT.  One double comes back to the host.
int objective(smg_membrane* m, const double* dx, double step, double* f)
{
    const smg_membrane_params& p = m->p;
    hipStream_t st = m->stream;
    HIPCHK(launch_membrane_trial(m->nV, m->qdot.p, dx, step, m->qdot0.p, m->pos0.p, m->fext.p, m->mass0.p, p.mass_scale, p.dt, m->qdotT.p, m->posT.p,
                                 m->terms.p + m->nF, st));
    HIPCHK(launch_membrane_faces_material(m->material, 0, m->nF, m->F.p, m->posT.p, m->V0.p, m->rest.p, p.thickness, m->alpha, m->beta, p.eig_floor,
                                          p.eig_value, m->terms.p, nullptr, nullptr, st));
    HIPCHK(launch_fixed_sum(m->terms.p, m->nF + m->nV, m->part.p, m->E.p, st));
    HIPCHK(hipMemcpyAsync(f, m->E.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_membrane_params* pp, smg_membrane** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_membrane_create";
    if (!h || !V || !F || !pp || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 3, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (const char* why = bad_params(*pp)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);

    std::unique_ptr<smg_membrane> m(new smg_membrane());
    m->nV = nV; m->nF = nF; m->p = *pp;
    lame(*pp, m->alpha, m->beta);
    if (int rc = m->open(who)) return rc;
    if (int rc = m->clone(who, h, 0)) return rc;
    hipStream_t st = m->stream;

    MembraneLists L;
    membrane_lists(F, nF, nV, L);
    m->nB = (int)L.bcol.size();
    if (int rc = upload_faces(F, nF, nV, m->F, m->m_ptr, m->m_idx)) return rc;
    HIPCHK(m->brow.upload(L.brow));
    HIPCHK(m->bcol.upload(L.bcol));
    HIPCHK(m->bptr.upload(L.bptr));
    HIPCHK(m->c_ptr.upload(L.c_ptr));
    HIPCHK(m->c_src.upload(L.c_src));
    HIPCHK(m->V0.upload(std::vector<double>(V, V + 3 * (size_t)nV)));

    const size_t n3 = 3 * (size_t)nV, nf = (size_t)nF, nval = 9 * (size_t)m->nB;
    for (DevBuf<double>* d : {&m->pos, &m->qdot, &m->posT, &m->qdotT, &m->pos0, &m->qdot0, &m->fext, &m->b, &m->dx, &m->zero}) HIPCHK(d->alloc(n3));
    HIPCHK(m->rest.alloc(5 * nf));
    HIPCHK(m->mass0.alloc((size_t)nV));
    HIPCHK(m->Hval.alloc(nval));
    HIPCHK(m->G.alloc(9 * nf));
    HIPCHK(m->H.alloc(45 * nf));
    HIPCHK(m->Qn.alloc(6 * nf));
    HIPCHK(m->terms.alloc(nf + (size_t)nV));
    HIPCHK(m->part.alloc((size_t)fixed_sum_groups(nF + nV)));
    HIPCHK(m->E.alloc(2));
    for (DevBuf<double>* d : {&m->qdot, &m->qdot0, &m->fext, &m->zero}) HIPCHK(hipMemsetAsync(d->p, 0, n3 * sizeof(double), st));
    HIPCHK(hipMemcpyAsync(m->pos.p, m->V0.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, st));

    // the rest constants, the mass, and H of the rest pose: the matrix of the first (pattern-setting) precompute
    HIPCHK(launch_membrane_rest(nF, m->F.p, m->V0.p, pp->thickness, m->rest.p, st));
    HIPCHK(launch_membrane_pressure(nV, nF, m->F.p, m->V0.p, m->m_ptr.p, m->m_idx.p, pp->pressure, m->Qn.p, m->mass0.p, nullptr, st));
    if (int rc = assemble(m.get(), m->V0.p, m->qdot.p, m->qdot0.p)) return rc;
    std::vector<double> val(nval);
    HIPCHK(hipMemcpyAsync(val.data(), m->Hval.p, nval * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> ptr(n3 + 1), col(nval);
    for (int i = 0; i < nV; i++) {
        const int first = L.bptr[i], cnt = L.bptr[i + 1] - first;
        for (int l = 0; l < 3; l++) {
            const size_t row0 = 9 * (size_t)first + (size_t)l * 3 * cnt;
            ptr[3 * (size_t)i + l] = (int)row0;
            for (int s = 0; s < cnt; s++)
                for (int c = 0; c < 3; c++) col[row0 + 3 * (size_t)s + c] = 3 * L.bcol[first + s] + c;
        }
    }
    ptr[n3] = (int)nval;
    if (int rc = smg_precompute(m->handle[0], (int)n3, ptr.data(), col.data(), val.data(), nullptr, 0)) return rc;
    if (smg_hierarchy_block_size(m->handle[0]) != 3) return fail(SMG_ERR_INVALID, "%s: the precompute did not take the block path", who);
    *out = m.release();
    return SMG_OK;
}

int step_impl(smg_membrane* m, const smg_solve_opts* opts, double* objective_his, double* alpha, int* cycles, int* n_newton)
{
    if (n_newton) *n_newton = 0;
    if (!m) return fail(SMG_ERR_INVALID, "smg_membrane_step: null object");
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    const smg_membrane_params& p = m->p;
    const int nV = m->nV, n3 = 3 * nV;
    const size_t vec = (size_t)n3 * sizeof(double);
    const smg_solve_opts so = opts_or_default(opts, 2e-1);      // the reference's mg_tolerance (main.cpp)

    HIPCHK(hipMemcpyAsync(m->pos0.p, m->pos.p, vec, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(m->qdot0.p, m->qdot.p, vec, hipMemcpyDeviceToDevice, st));
    HIPCHK(launch_membrane_pressure(nV, m->nF, m->F.p, m->pos.p, m->m_ptr.p, m->m_idx.p, p.pressure, m->Qn.p, nullptr, m->fext.p, st));
    double f0 = 0.0;
    if (int rc = objective(m, nullptr, 0.0, &f0)) return rc;
    if (objective_his) objective_his[0] = f0;
    if (!std::isfinite(f0)) return fail(SMG_ERR_NONFINITE, "smg_membrane_step: the objective of the state is not finite (a face with det a <= 0?)");

    for (int i = 0; i < p.newton_iters; i++) {
        if (int rc = assemble(m, m->pos.p, m->qdot.p, m->qdot0.p)) return rc;
        if (int rc = smg_precompute_values_device(m->handle[0], m->Hval.p)) return rc;
        if (int rc = inner_solve(m->handle[0], m->pcg, m->b.p, n3, nullptr, 0, m->zero.p, n3, 1, so, m->dx.p, n3, cycles ? cycles + i : nullptr)) return rc;
        double bdx = 0.0;
        HIPCHK(launch_membrane_dot3(nV, m->b.p, m->dx.p, m->terms.p, st));
        HIPCHK(launch_fixed_sum(m->terms.p, nV, m->part.p, m->E.p + 1, st));
        HIPCHK(hipMemcpyAsync(&bdx, m->E.p + 1, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // the reference's acceptance test: s = f0 + c b . dx with b the NEGATIVE gradient
        const double s = f0 + p.ls_c * bdx;
        double a = 1.0, taken = 0.0;
        while (a > p.ls_min_alpha) {
            double ft = 0.0;
            if (int rc = objective(m, m->dx.p, a, &ft)) return rc;
            if (ft <= s) {
                std::swap(m->qdot, m->qdotT);
                std::swap(m->pos, m->posT);
                f0 = ft;
                taken = a;
                break;
            }
            a *= p.ls_shrink;
        }
        if (taken == 0.0 && i == 0) {      // pos = pos0 + dt qdot also when the search gave up (later iterations are there already)
            HIPCHK(launch_membrane_trial(nV, m->qdot.p, nullptr, 0.0, m->qdot0.p, m->pos0.p, m->fext.p, m->mass0.p, p.mass_scale, p.dt, m->qdotT.p,
                                         m->posT.p, m->terms.p + m->nF, st));
            std::swap(m->pos, m->posT);
        }
        if (alpha) alpha[i] = taken;
        if (objective_his) objective_his[i + 1] = f0;
        if (n_newton) *n_newton = i + 1;
        if (!std::isfinite(f0)) return fail(SMG_ERR_NONFINITE, "smg_membrane_step: non-finite objective after Newton iteration %d", i);
    }
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int state_impl(smg_membrane* m, double* pos, double* qdot, const double* pos_in, const double* qdot_in, int memspace, bool set)
{
    if (!m || bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "smg_membrane_%s_state: bad arguments", set ? "set" : "get");
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    const size_t vec = 3 * (size_t)m->nV * sizeof(double);
    if (set) {
        const hipMemcpyKind in = copy_in(memspace);
        HIPCHK(hipMemcpyAsync(m->pos.p, pos_in ? pos_in : m->V0.p, vec, pos_in ? in : hipMemcpyDeviceToDevice, st));
        if (qdot_in) HIPCHK(hipMemcpyAsync(m->qdot.p, qdot_in, vec, in, st));
        else HIPCHK(hipMemsetAsync(m->qdot.p, 0, vec, st));
    } else {
        const hipMemcpyKind back = copy_out(memspace);
        if (pos) HIPCHK(hipMemcpyAsync(pos, m->pos.p, vec, back, st));
        if (qdot) HIPCHK(hipMemcpyAsync(qdot, m->qdot.p, vec, back, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

}  // namespace

extern "C" void smg_membrane_params_default(smg_membrane_params* p)
{
    if (!p) return;
    p->young = 6e6; p->poisson = 0.5; p->thickness = 0.1; p->mass_scale = 1000.0; p->dt = 1e-3; p->pressure = 1e6; p->newton_iters = 10;
    p->ls_c = 1e-8; p->ls_shrink = 0.5; p->ls_min_alpha = 1e-8; p->eig_floor = 1e-6; p->eig_value = 1e-3;
}

extern "C" int smg_membrane_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_membrane_params* p, smg_membrane** out)
{
    return guarded("smg_membrane_create", [&]() { return create_impl(h, V, nV, F, nF, p, out); });
}

extern "C" void smg_membrane_destroy(smg_membrane* m) { delete m; }

extern "C" long long smg_membrane_device_bytes(const smg_membrane* m)
{
    if (!m) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*m, m->F, m->m_ptr, m->m_idx, m->brow, m->bcol, m->bptr, m->c_ptr, m->c_src, m->V0, m->rest, m->mass0, m->pos, m->qdot, m->posT,
                        m->qdotT, m->pos0, m->qdot0, m->fext, m->b, m->dx, m->zero, m->Hval, m->G, m->H, m->Qn, m->terms, m->part, m->E);
}

extern "C" int smg_membrane_set_state(smg_membrane* m, const double* pos, const double* qdot, int memspace)
{
    return guarded("smg_membrane_set_state", [&]() { return state_impl(m, nullptr, nullptr, pos, qdot, memspace, true); });
}

extern "C" int smg_membrane_get_state(smg_membrane* m, double* pos, double* qdot, int memspace)
{
    return guarded("smg_membrane_get_state", [&]() { return state_impl(m, pos, qdot, nullptr, nullptr, memspace, false); });
}

extern "C" int smg_membrane_set_solver(smg_membrane* m, int pcg)
{
    if (!m) return fail(SMG_ERR_INVALID, "null membrane object");
    latch_solver(m->pcg, pcg);
    return SMG_OK;
}

extern "C" int smg_membrane_set_material(smg_membrane* m, int material)
{
    if (!m) return fail(SMG_ERR_INVALID, "smg_membrane_set_material: null object");
    if (material < 0 || material > 2)
        return fail(SMG_ERR_INVALID, "smg_membrane_set_material: material %d is not 0 (neo-Hookean), 1 (StVK) or 2 (tension-field StVK)", material);
    m->material = material;
    return SMG_OK;
}

extern "C" int smg_membrane_material(const smg_membrane* m) { return m ? m->material : 0; }

extern "C" int smg_membrane_step(smg_membrane* m, const smg_solve_opts* opts, double* objective_his, double* alpha, int* cycles, int* n_newton)
{
    return guarded("smg_membrane_step", [&]() { return step_impl(m, opts, objective_his, alpha, cycles, n_newton); });
}

extern "C" int smg_membrane_lists(const int* F, int nF, int nV, int* n_blocks, int* n_contrib, int* bptr, int* bcol, int* c_ptr, int* c_src)
{
    return guarded("smg_membrane_lists", [&]() -> int {
        if (!F || nF <= 0 || nV <= 0) return fail(SMG_ERR_INVALID, "smg_membrane_lists: bad arguments");
        if (int rc = check_faces("smg_membrane_lists", F, nF, nV)) return rc;
        MembraneLists L;
        membrane_lists(F, nF, nV, L);
        if (n_blocks) *n_blocks = (int)L.bcol.size();
        if (n_contrib) *n_contrib = (int)L.c_src.size();
        if (bptr) std::copy(L.bptr.begin(), L.bptr.end(), bptr);
        if (bcol) std::copy(L.bcol.begin(), L.bcol.end(), bcol);
        if (c_ptr) std::copy(L.c_ptr.begin(), L.c_ptr.end(), c_ptr);
        if (c_src) std::copy(L.c_src.begin(), L.c_src.end(), c_src);
        return SMG_OK;
    });
}

namespace {

// W (and G, H: 9 and 45 planes of nF) of every face at P; material 0 reads the first five of the eight rest constants
template <bool DERIVS>
double face_host(int material, const double (&q)[9], const double (&r)[8], const smg_membrane_params& p, double alpha, double beta, double (&g)[9],
                 double (&h)[45])
{
    if (material == 1) return membrane_face_mat<1, DERIVS>(q, r, p.thickness, alpha, beta, g, h);
    if (material == 2) return membrane_face_mat<2, DERIVS>(q, r, p.thickness, alpha, beta, g, h);
    const double r5[5] = {r[0], r[1], r[2], r[3], r[4]};
    return membrane_face<DERIVS>(q, r5, alpha, beta, g, h);
}

void faces_host(const double* V0, const double* P, const int* F, int nF, const smg_membrane_params& p, int material, int fix, double* W, double* G, double* H)
{
    double alpha, beta;
    lame(p, alpha, beta);
    const size_t nf = (size_t)nF;
    for (int f = 0; f < nF; f++) {
        double q0[9], q[9], r[8], g[9], h[45];
        for (int j = 0; j < 3; j++)
            for (int d = 0; d < 3; d++) {
                q0[3 * j + d] = V0[3 * (size_t)F[3 * (size_t)f + j] + d];
                q[3 * j + d] = P[3 * (size_t)F[3 * (size_t)f + j] + d];
            }
        mem_rest_consts(q0, p.thickness, r);
        if (!G) { W[f] = face_host<false>(material, q, r, p, alpha, beta, g, h); continue; }
        W[f] = face_host<true>(material, q, r, p, alpha, beta, g, h);
        for (int e = 0; e < 9; e++) G[e * nf + f] = g[e];
        if (!H) continue;
        if (fix) membrane_fix(h, p.eig_floor, p.eig_value);
        for (int e = 0; e < 45; e++) H[e * nf + f] = h[e];
    }
}

}  // namespace

extern "C" int smg_membrane_faces_host(const double* V0, const double* P, int nV, const int* F, int nF, const smg_membrane_params* p, int fix,
                                       double* W, double* G, double* H)
{
    return guarded("smg_membrane_faces_host", [&]() -> int {
        if (!V0 || !P || !F || !p || !W || nV <= 0 || nF <= 0 || (H && !G)) return fail(SMG_ERR_INVALID, "smg_membrane_faces_host: bad arguments");
        if (const char* why = bad_params(*p)) return fail(SMG_ERR_INVALID, "smg_membrane_faces_host: %s", why);
        if (int rc = check_mesh("smg_membrane_faces_host", V0, nV, F, nF, false)) return rc;
        faces_host(V0, P, F, nF, *p, 0, fix, W, G, H);
        return SMG_OK;
    });
}

extern "C" int smg_membrane_faces_host_material(const double* V0, const double* P, int nV, const int* F, int nF, const smg_membrane_params* p,
                                                int material, int fix, double* W, double* G, double* H)
{
    return guarded("smg_membrane_faces_host_material", [&]() -> int {
        const char* who = "smg_membrane_faces_host_material";
        if (!V0 || !P || !F || !p || !W || nV <= 0 || nF <= 0 || (H && !G)) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        if (material < 0 || material > 2)
            return fail(SMG_ERR_INVALID, "%s: material %d is not 0 (neo-Hookean), 1 (StVK) or 2 (tension-field StVK)", who, material);
        if (const char* why = bad_params(*p)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
        if (int rc = check_mesh(who, V0, nV, F, nF, false)) return rc;
        faces_host(V0, P, F, nF, *p, material, fix, W, G, H);
        return SMG_OK;
    });
}
