// smg_local_global.hpp -- the control flow of a local / global alternation (smg_arap_solve, smg_param_arap) and nothing
// else: no HIP, no library symbol, so tests/local_global_driver.cpp drives it with scripted energies.
//   local(t, with_rhs, &E_t)   enqueues the local step and the energy's sum of iterate t -- with_rhs: and what the global step reads --, synchronises
//                              once and leaves E_t on the host; non-zero: that code is returned, *n_iter untouched
//   global(t, &entries)        the warm-started inner solve, the buffer swap and what follows it; non-zero ends the loop with that code
// For t = 0, 1, ...: local(t, t < max_iter); energy_his[t] = E_t; a non-finite E_t ends with LOCAL_GLOBAL_NONFINITE; t == max_iter ends; for
// t > 0 and rel_tol > 0, E_prev - E_t <= rel_tol |E_prev| ends (an increase too); global(t), cycles[t] = entries.  Every end leaves *n_iter = t.
// energy_his (max_iter + 1 entries), cycles (max_iter) and n_iter may each be null.
#pragma once
#include <cmath>

namespace smg {

constexpr int LOCAL_GLOBAL_NONFINITE = 1;   // no error code of the library is positive: the caller words the message

template <class Local, class Global>
int local_global(int max_iter, double rel_tol, Local&& local, Global&& global, double* energy_his, int* cycles, int* n_iter)
{
    auto end = [n_iter](int t, int rc) { if (n_iter) *n_iter = t; return rc; };
    double E_prev = 0.0;
    for (int t = 0;; t++) {
        double E_t = 0.0;
        if (int rc = local(t, t < max_iter, &E_t)) return rc;
        if (energy_his) energy_his[t] = E_t;
        if (!std::isfinite(E_t)) return end(t, LOCAL_GLOBAL_NONFINITE);
        if (t == max_iter) return end(t, 0);
        if (t > 0 && rel_tol > 0.0 && E_prev - E_t <= rel_tol * std::fabs(E_prev)) return end(t, 0);
        E_prev = E_t;
        int entries = 0;
        if (int rc = global(t, &entries)) return end(t, rc);
        if (cycles) cycles[t] = entries;
    }
}

}  // namespace smg
