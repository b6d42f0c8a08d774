// smg_sinkhorn.cpp -- the host twin of heat-kernel optimal transport on a mesh (include/smg.h: smg_sinkhorn_host; Solomon
// et al. 2015, Convolutional Wasserstein Distances): the pointwise operations of the Sinkhorn iterations -- the scaling update with its marginal
// error, the right-hand side of a substep, the value's terms, the weighted geometric mean of a barycentre -- on caller arrays, with the
// fixed-order sums of their planes.  No GPU is used.  The arithmetic is csrc/smg_sinkhorn_inl.hpp; tests/sinkhorn_np.py restates it in numpy.
#include <cmath>
#include <vector>

#include "smg_internal.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_sinkhorn_inl.hpp"

using namespace smg;

namespace smg {

int sinkhorn_check_operands(const char* who, int op, int nV, int nF, int k, int k_in, const int* F, const double* V, const double* y, const double* r,
                            const double* mu, const double* mu1, const double* sr, const double* alphas, double floor, const double* out)
{
    if (op < SMG_SINKHORN_SCALE || op > SMG_SINKHORN_GEOMEAN || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool scale = op == SMG_SINKHORN_SCALE, value = op == SMG_SINKHORN_VALUE, geo = op == SMG_SINKHORN_GEOMEAN;
    if (!y || (op != SMG_SINKHORN_SUBSTEP && (!r || !mu)) || (value && !mu1) || ((scale || geo) && !sr) || (geo && !alphas))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if ((scale || geo) && k_in < 1) return fail(SMG_ERR_INVALID, "%s: k_in = %d, at least one column is needed", who, k_in);
    if ((scale || geo) && (!std::isfinite(floor) || floor < 0.0)) return fail(SMG_ERR_INVALID, "%s: kernel_floor = %g, a finite value >= 0 is needed", who, floor);
    return check_faces(who, F, nF, nV);
}

}  // namespace smg

extern "C" int smg_sinkhorn_host(int op, int nV, int nF, int k, int k_in, const int* F, const double* V, const double* y, const double* r, const double* mu,
                                 const double* mu1, const double* sr, const double* alphas, double floor, double* out)
{
    return guarded("smg_sinkhorn_host", [&]() -> int {
        const char* who = "smg_sinkhorn_host";
        if (int rc = sinkhorn_check_operands(who, op, nV, nF, k, k_in, F, V, y, r, mu, mu1, sr, alphas, floor, out)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk;
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        std::vector<double> Af(f), m(n);
        fluid_host_mass(nV, nF, F, V, mp.data(), mi.data(), Af.data(), m.data());
        const double A = flow_host_sum(m.data(), nV);
        switch (op) {
            case SMG_SINKHORN_SCALE:
                sinkhorn_host_scale(nV, k, k_in, y, r, mu, sr, floor, A, out, out + nk, out + 2 * nk);
                for (size_t c = 0; c < kk; c++) {
                    out[3 * nk + c] = flow_host_sum(out + c * n, nV);
                    out[3 * nk + kk + c] = flow_host_sum(out + nk + c * n, nV);
                }
                out[3 * nk + 2 * kk] = flow_host_sum(out + 2 * nk, (int)nk);
                break;
            case SMG_SINKHORN_SUBSTEP:
                sinkhorn_host_substep(nV, k, m.data(), y, out, out + nk);
                out[2 * nk] = flow_host_sum(out + nk, (int)nk);
                break;
            case SMG_SINKHORN_VALUE:
                sinkhorn_host_value(nV, k, m.data(), mu, mu1, r, y, out, out + nk, out + 2 * nk);
                for (size_t c = 0; c < kk; c++) out[3 * nk + c] = flow_host_sum(out + c * n, nV);
                break;
            default: {
                const size_t K = kk * (size_t)k_in, nK = n * K;
                double *rn = out, *bary = out + nK, *chg = bary + nk, *rsq = chg + nk, *s = rsq + nK;
                sinkhorn_host_geomean(nV, k, k_in, m.data(), y, r, mu, sr, alphas, floor, A, rn, bary, chg, rsq);
                for (size_t c = 0; c < K; c++) s[c] = flow_host_sum(rn + c * n, nV);
                for (size_t q = 0; q < kk; q++) {
                    s[K + q] = flow_host_sum(chg + q * n, nV);
                    s[K + kk + q] = flow_host_sum(bary + q * n, nV);
                }
                s[K + 2 * kk] = flow_host_sum(rsq, (int)nK);
                break;
            }
        }
        return SMG_OK;
    });
}
