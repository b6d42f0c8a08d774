// smg_wave_born_inl.hpp -- the per-entry arithmetic of the wave object's tangent (Born) run, in registers (csrc/smg_wave_born_device.hip,
// smg_wave_born_host; include/smg.h: smg_wave_gauss_newton).  Layouts as in smg_wave_inl.hpp: vertex blocks are column-major
// nV x k, term planes are k planes of nV; fd = fac d is nV x d_cols, d_cols 1 or k, and column c reads its column c % d_cols.
//
//   born      x = b + fd e;  b = x;  rsq = x x                       off the known rows; a known row keeps its b and rsq (0.0 in a run)
//   plane     fd = fac d,  fac = (-2.0 mt) / speed                   formed on the host, one multiply per entry
// Only + and * occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit for bit.
#pragma once
#include <cstddef>

#include "smg_wave_inl.hpp"

namespace smg {

SMG_ARAP_HD double wave_born(double b, double fd, double e) { return b + fd * e; }

// ---- the host twin (smg_wave_born_host): the kernel's loop on caller arrays, with the layouts of smg_debug_wave_born (include/smg.h) ---------------
// fac (nV), d (nV x d_cols, leading dimension ldd) -> fd (nV x d_cols)
inline void wave_born_host_plane(int nV, int d_cols, const double* fac, const double* d, int ldd, double* fd)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < d_cols; c++)
        for (size_t i = 0; i < n; i++) fd[(size_t)c * n + i] = fac[i] * d[(size_t)c * (size_t)ldd + i];
}

// fd (nV x d_cols), e (nV x k); b (nV x k) and rsq (k planes of nV) in place
inline void wave_born_host(int nV, int k, int d_cols, const int* known, const double* fd, const double* e, double* b, double* rsq)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            if (known && known[i]) continue;
            const size_t o = (size_t)c * n + i;
            const double x = wave_born(b[o], fd[(size_t)(c % d_cols) * n + i], e[o]);
            b[o] = x;
            rsq[o] = x * x;
        }
}

}  // namespace smg
