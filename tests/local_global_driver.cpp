// local_global_driver.cpp -- drives smg::local_global (csrc/smg_local_global.hpp) with scripted energies and a scripted inner solve.  One
// translation unit, its own main; tests/test_local_global.py compiles it with -fsanitize=address,undefined and runs it.  energy_his and
// cycles are heap arrays of exactly max_iter + 1 and max_iter entries, so a write past either is a sanitizer report.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "smg_local_global.hpp"

namespace {

const double QNAN = std::numeric_limits<double>::quiet_NaN();
const double SENTINEL = -777.0;
int failures = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("  FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

struct Run {
    int rc = 0, n_iter = -99;
    std::vector<double> his;          // what the loop left in energy_his (SENTINEL: untouched)
    std::vector<int> cycles;          // ... in cycles (-99: untouched)
    std::vector<int> with_rhs;        // the flag of every local call
    std::vector<int> solves;          // the t of every global call
};

// energies[t] is what local(t) reports; the solve at t returns fail_rc when t == fail_at, else 0 with 10 + t entries.
// outputs == false: the three output pointers are null.
Run run(const std::vector<double>& energies, int max_iter, double rel_tol, int fail_at = -1, int fail_rc = 0, bool outputs = true)
{
    Run r;
    double* his = new double[(size_t)max_iter + 1];
    int* cyc = new int[(size_t)max_iter];
    for (int t = 0; t <= max_iter; t++) his[t] = SENTINEL;
    for (int t = 0; t < max_iter; t++) cyc[t] = -99;
    auto local = [&](int t, bool with_rhs, double* E) {
        r.with_rhs.push_back(with_rhs ? 1 : 0);
        if (t != (int)r.with_rhs.size() - 1 || t >= (int)energies.size()) { std::printf("  FAILED: local(%d) is off the script\n", t); failures++; return -99; }
        *E = energies[(size_t)t];
        return 0;
    };
    auto global = [&](int t, int* entries) {
        r.solves.push_back(t);
        if (t == fail_at) return fail_rc;
        *entries = 10 + t;
        return 0;
    };
    r.rc = smg::local_global(max_iter, rel_tol, local, global, outputs ? his : nullptr, outputs ? cyc : nullptr, outputs ? &r.n_iter : nullptr);
    r.his.assign(his, his + max_iter + 1);
    r.cycles.assign(cyc, cyc + max_iter);
    delete[] his;
    delete[] cyc;
    return r;
}

bool history_is(const Run& r, const std::vector<double>& want)      // the first entries are `want` (NaN matches NaN), the rest untouched
{
    for (size_t t = 0; t < r.his.size(); t++) {
        const double w = t < want.size() ? want[t] : SENTINEL;
        if (!(r.his[t] == w || (std::isnan(r.his[t]) && std::isnan(w)))) return false;
    }
    return want.size() <= r.his.size();
}

bool cycles_are(const Run& r, int n)                                // the first n are the script's 10 + t, the rest untouched
{
    for (size_t t = 0; t < r.cycles.size(); t++)
        if (r.cycles[t] != ((int)t < n ? 10 + (int)t : -99)) return false;
    return true;
}

}  // namespace

int main()
{
    std::printf("a: max_iter ends\n");
    {
        const Run r = run({8, 4, 2, 1}, 3, 0.0);
        EXPECT(r.rc == 0 && r.n_iter == 3);
        EXPECT(history_is(r, {8, 4, 2, 1}));
        EXPECT((r.with_rhs == std::vector<int>{1, 1, 1, 0}));
        EXPECT((r.solves == std::vector<int>{0, 1, 2}) && cycles_are(r, 3));
    }
    std::printf("b: a relative drop equal to rel_tol stops\n");
    {
        const Run r = run({8, 4, 2, 1, 0.5}, 20, 0.5);
        EXPECT(r.rc == 0 && r.n_iter == 1);
        EXPECT(history_is(r, {8, 4}));
        EXPECT((r.solves == std::vector<int>{0}) && cycles_are(r, 1));
        EXPECT((r.with_rhs == std::vector<int>{1, 1}));
    }
    std::printf("c: the drop is relative to the previous energy\n");
    {
        const Run r = run({8, 4, 3, 2.9}, 20, 0.4);
        EXPECT(r.rc == 0 && r.n_iter == 2);
        EXPECT(history_is(r, {8, 4, 3}));
        EXPECT((r.solves == std::vector<int>{0, 1}) && cycles_are(r, 2));
    }
    std::printf("d: an increase stops only under a positive rel_tol\n");
    {
        const Run r0 = run({8, 9, 7, 6}, 3, 0.0);
        EXPECT(r0.rc == 0 && r0.n_iter == 3 && history_is(r0, {8, 9, 7, 6}) && cycles_are(r0, 3));
        const Run r1 = run({8, 9, 7, 6}, 3, 0.1);
        EXPECT(r1.rc == 0 && r1.n_iter == 1 && history_is(r1, {8, 9}) && cycles_are(r1, 1));
        EXPECT((r1.solves == std::vector<int>{0}));
    }
    std::printf("e: max_iter 0\n");
    {
        const Run r = run({5}, 0, 0.0);
        EXPECT(r.rc == 0 && r.n_iter == 0);
        EXPECT(history_is(r, {5}) && r.his.size() == 1);
        EXPECT((r.with_rhs == std::vector<int>{0}) && r.solves.empty());
        const Run r2 = run({5}, 0, 0.3);
        EXPECT(r2.rc == 0 && r2.n_iter == 0 && r2.solves.empty());
    }
    std::printf("f: a non-finite energy\n");
    {
        const Run r = run({8, 4, QNAN, 1}, 5, 0.0);
        EXPECT(r.rc == smg::LOCAL_GLOBAL_NONFINITE && r.n_iter == 2);
        EXPECT(history_is(r, {8, 4, QNAN}) && std::isnan(r.his[2]));
        EXPECT((r.solves == std::vector<int>{0, 1}) && cycles_are(r, 2));
        const Run r0 = run({INFINITY}, 3, 0.0);                    // at iteration 0: no solve is reached
        EXPECT(r0.rc == smg::LOCAL_GLOBAL_NONFINITE && r0.n_iter == 0 && r0.solves.empty() && cycles_are(r0, 0));
        const Run rl = run({8, 4, 2, QNAN}, 3, 0.0);               // at t == max_iter the refusal comes first
        EXPECT(rl.rc == smg::LOCAL_GLOBAL_NONFINITE && rl.n_iter == 3 && std::isnan(rl.his[3]));
    }
    std::printf("g: a failing inner solve\n");
    {
        const Run r = run({8, 4, 2, 1}, 3, 0.0, 1, -3);
        EXPECT(r.rc == -3 && r.n_iter == 1);
        EXPECT(history_is(r, {8, 4}));
        EXPECT((r.solves == std::vector<int>{0, 1}) && cycles_are(r, 1));     // cycles[0] set, cycles[1] untouched
    }
    std::printf("h: null outputs\n");
    {
        const Run r = run({8, 4, 2, 1}, 3, 0.0, -1, 0, false);
        EXPECT(r.rc == 0 && r.n_iter == -99);
        EXPECT(history_is(r, {}) && cycles_are(r, 0));
        EXPECT((r.with_rhs == std::vector<int>{1, 1, 1, 0}) && (r.solves == std::vector<int>{0, 1, 2}));
        const Run rn = run({8, QNAN}, 3, 0.0, -1, 0, false);
        EXPECT(rn.rc == smg::LOCAL_GLOBAL_NONFINITE && rn.solves.size() == 1);
    }
    if (failures) { std::printf("LOCAL_GLOBAL_DRIVER: %d check(s) failed\n", failures); return 1; }
    std::printf("LOCAL_GLOBAL_DRIVER OK\n");
    return 0;
}
