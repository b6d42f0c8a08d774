// smg_mesh_object.cpp -- the shared part of the objects built on a mesh and a caller's hierarchy (smg_mesh_object.hpp).
#include "smg_mesh_object.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "smg_bsr3.hpp"

namespace smg {

double double_area(const double* V, const int* F, int f)
{
    const double* a = V + 3 * (size_t)F[3 * (size_t)f];
    const double* b = V + 3 * (size_t)F[3 * (size_t)f + 1];
    const double* c = V + 3 * (size_t)F[3 * (size_t)f + 2];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    return std::sqrt(wx * wx + wy * wy + wz * wz);
}

int components(const int* F, int nF, int nV)
{
    std::vector<int> parent(nV);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (size_t f = 0; f < (size_t)nF; f++)
        for (int c = 1; c < 3; c++) {
            const int a = find(F[3 * f]), b = find(F[3 * f + c]);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
    int n = 0;
    for (int v = 0; v < nV; v++) n += find(v) == v ? 1 : 0;
    return n;
}

int level0_rows(const smg_hierarchy* h)
{
    if (h->n_levels >= 2) return h->lv[1].P_full.nr > 0 ? h->lv[1].P_full.nr : -1;
    return h->lv[0].V.empty() ? -1 : (int)(h->lv[0].V.size() / 3);
}

int copy_prolongations(const smg_hierarchy* src, smg_hierarchy* dst)
{
    for (int lv = 1; lv < src->n_levels; lv++) {
        Csr P = src->lv[lv].P_full;
        if (int rc = set_prolong(dst, lv, std::move(P))) return rc;
    }
    return SMG_OK;
}

long long handle_bytes(const smg_hierarchy* h)
{
    long long total = 0;
    if (h)
        for (const auto& e : device_byte_entries(h)) total += e.second;
    return total;
}

int check_hierarchy(const char* who, const smg_hierarchy* h, int dofs, int nV)
{
    if (h->union_m > 0) return fail(SMG_ERR_INVALID, "%s: union handles are not supported", who);
    const int rows = level0_rows(h);
    Csr Pv;
    if (dofs == 1) {
        if (h->bs == 3 || h->block_mode == 3 || (h->n_levels >= 2 && h->lv[1].P_full.nr > 0 && kron3_factor(h->lv[1].P_full, Pv)))
            return fail(SMG_ERR_INVALID, "%s: block (3-DOF) hierarchies are not supported", who);
        if (rows != nV) return fail(SMG_ERR_INVALID, "%s: nV = %d, but level 0 of the hierarchy has %d rows", who, nV, rows);
        return SMG_OK;
    }
    if (h->block_mode == 0 || h->n_levels < 2 || rows <= 0 || !kron3_factor(h->lv[1].P_full, Pv))
        return fail(SMG_ERR_INVALID, "%s: a block (3-DOF) hierarchy is needed (smg_mg_precompute_block; prolongations Pv (x) I_3)", who);
    for (int lv = 2; lv < h->n_levels; lv++)
        if (!kron3_factor(h->lv[lv].P_full, Pv)) return fail(SMG_ERR_INVALID, "%s: the prolongation of level %d is not Pv (x) I_3", who, lv);
    if ((long long)rows != 3LL * nV) return fail(SMG_ERR_INVALID, "%s: nV = %d, but level 0 of the hierarchy has %d rows (3 nV expected)", who, nV, rows);
    return SMG_OK;
}

int check_faces(const char* who, const int* F, int nF, int nV)
{
    for (size_t i = 0; i < (size_t)nF * 3; i++)
        if (F[i] < 0 || F[i] >= nV) return fail(SMG_ERR_INVALID, "%s: face index out of range", who);
    return SMG_OK;
}

int check_mesh(const char* who, const double* V, int nV, const int* F, int nF, bool connected, double* area2)
{
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    double sum = 0.0;
    for (int f = 0; f < nF; f++) {
        const double dA = double_area(V, F, f);
        if (!(dA > 0.0)) return fail(SMG_ERR_INVALID, "%s: face %d has zero double area", who, f);
        sum += dA;
    }
    if (area2) *area2 = sum;
    for (size_t i = 0; i < (size_t)nV * 3; i++)
        if (!std::isfinite(V[i])) return fail(SMG_ERR_INVALID, "%s: non-finite vertex coordinate", who);
    if (connected)
        if (const int nc = components(F, nF, nV); nc != 1)
            return fail(SMG_ERR_INVALID, "%s: the mesh has %d connected components (vertices in no face count)", who, nc);
    return SMG_OK;
}

int MeshObject::open(const char* who)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SMG_ERR_NO_DEVICE, "%s: no HIP device: libsmg has no CPU fallback", who);
    HIPCHK(hipGetDevice(&device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return SMG_OK;
}

int MeshObject::clone(const char* who, const smg_hierarchy* src, int slot)
{
    HierarchyOwner own(smg_hierarchy_create(src->n_levels));
    if (!own.h) return fail(SMG_ERR_ALLOC, "%s: out of memory", who);
    if (int rc = copy_prolongations(src, own.h)) return rc;
    if (int rc = smg_hierarchy_set_stream(own.h, stream)) return rc;
    handle[slot] = own.release();
    return SMG_OK;
}

void MeshObject::quiesce()
{
    if (stream) (void)hipStreamSynchronize(stream);
    for (int s = 1; s >= 0; s--)
        if (handle[s]) { smg_hierarchy_destroy(handle[s]); handle[s] = nullptr; }
}

int cotan_system(const int* F, int nF, int nV, const double* d_V, int voronoi, double c_mass, double c_L, hipStream_t st, CotanSystem& S, bool val,
                 DevBuf<double>* keep_L)
{
    smg_assembler* a = nullptr;
    if (int rc = smg_assembler_create(F, nF, nV, &a)) return rc;
    struct AsmOwner { smg_assembler* a; ~AsmOwner() { smg_assembler_destroy(a); } } own_a{a};
    int nnz = 0;
    smg_assembler_pattern(a, &nnz, nullptr, nullptr);
    S.ptr.resize((size_t)nV + 1);
    S.col.resize((size_t)nnz);
    smg_assembler_pattern(a, nullptr, S.ptr.data(), S.col.data());
    DevBuf<double> dval, dL_own;
    DevBuf<double>& dL = keep_L ? *keep_L : dL_own;
    HIPCHK(dval.alloc((size_t)nnz));
    HIPCHK(dL.alloc((size_t)nnz));
    if (int rc = smg_assemble(a, d_V, voronoi, c_mass, c_L, dval.p, nullptr, dL.p, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    S.L.resize((size_t)nnz);
    S.val.resize(val ? (size_t)nnz : 0);
    if (val) HIPCHK(hipMemcpy(S.val.data(), dval.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(S.L.data(), dL.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
    return SMG_OK;
}

int inner_solve(smg_hierarchy* h, int pcg, const double* B, int ldb, const double* known, int ld_kv, const double* z0, int ld_z0, int k,
                const smg_solve_opts& o, double* z, int ld_z, int* entries)
{
    std::vector<double> his((size_t)std::max(1, o.max_iter));
    int n_his = 0, conv = 0;
    const int rc = (pcg ? smg_solve_pcg : smg_solve)(h, B, ldb, known, ld_kv, z0, ld_z0, k, SMG_DEVICE, &o, z, ld_z, his.data(), &n_his, &conv);
    if (rc == SMG_OK && entries) *entries = n_his;
    return rc;
}

smg_solve_opts opts_or_default(const smg_solve_opts* opts, double tol, int max_iter)
{
    if (opts) return *opts;
    smg_solve_opts so;
    smg_solve_opts_default(&so);
    so.tol = tol;
    if (max_iter > 0) so.max_iter = max_iter;
    return so;
}

int upload_faces(const int* F, int nF, int nV, DevBuf<int>& d_F, DevBuf<int>& d_ptr, DevBuf<int>& d_idx, std::vector<int>* mp, std::vector<int>* mi)
{
    std::vector<int> Fv(F, F + 3 * (size_t)nF), ptr, idx;
    vertex_corner_lists(Fv, nV, ptr, idx);
    HIPCHK(d_F.upload(Fv));
    HIPCHK(d_ptr.upload(ptr));
    HIPCHK(d_idx.upload(idx));
    if (mp) mp->swap(ptr);
    if (mi) mi->swap(idx);
    return SMG_OK;
}

}  // namespace smg
