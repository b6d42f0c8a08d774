// wave_gn_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the wave object's tangent (Born) run on exactly-sized heap
// arrays, so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: the loops of the host
// twin (smg::wave_born_host_plane and wave_born_host of csrc/smg_wave_born_inl.hpp, what smg_wave_born_host runs after its argument checks), on
// closed double pyramids of 255, 256, 257 and 2100 vertices -- the edges of a block of 256 lanes and several blocks -- free, and on their open
// fans clamped, with k = 1 and 3 columns and d_cols = 1 and 3 columns of the direction.  tests/test_wave_gn_host.py compiles it together with
// csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_wave_adjoint_inl.hpp"
#include "smg_wave_born_inl.hpp"

using namespace smg;

// the faces of a closed double pyramid: a ring of nV - 2 vertices, one apex above and one below; open: the upper fan alone, a ring of nV - 1
static void make_faces(int nV, bool open, std::vector<int>& F)
{
    const int ring = open ? nV - 1 : nV - 2, top = ring, bottom = ring + 1;
    F.clear();
    for (int i = 0; i < ring; i++) {
        const int j = (i + 1) % ring;
        F.insert(F.end(), {i, j, top});
        if (!open) F.insert(F.end(), {j, i, bottom});
    }
}

template <class T>
static std::unique_ptr<T[]> exact(size_t n)
{
    return std::unique_ptr<T[]>(new T[n]);
}

static bool run_case(int nV, bool open, int k, int d_cols)
{
    std::vector<int> Fv;
    make_faces(nV, open, Fv);
    const int nF = (int)Fv.size() / 3;
    const size_t n = (size_t)nV, kk = (size_t)k, nk = n * kk, dc = (size_t)d_cols;
    auto known = exact<int>(n);
    for (size_t i = 0; i < n; i++) known[i] = 0;
    if (open)
        for (int b : boundary_vertices(Fv.data(), nF, nV)) known[(size_t)b] = 1;
    auto mt = exact<double>(n), speed = exact<double>(n), fac = exact<double>(n);
    const int ldd = nV + 3;                                                   // the direction has a leading dimension of its own
    auto d = exact<double>((size_t)ldd * (dc - 1) + n), fd = exact<double>(n * dc), b = exact<double>(nk), e = exact<double>(nk), rsq = exact<double>(nk);
    for (size_t i = 0; i < n; i++) {
        mt[i] = 0.01 + 0.001 * (double)(i % 7);
        speed[i] = 1.0 + 0.25 * std::sin(0.1 * (double)i);
    }
    for (size_t c = 0; c < dc; c++)
        for (size_t i = 0; i < n; i++) d[c * (size_t)ldd + i] = c == 1 ? 0.0 : std::cos(0.3 * (double)i + (double)c);
    for (size_t c = 0; c < kk; c++)
        for (size_t i = 0; i < n; i++) {
            b[c * n + i] = known[i] ? 0.0 : std::sin(0.2 * (double)i - (double)c);
            e[c * n + i] = 0.1 + std::cos(0.05 * (double)i + 0.5 * (double)c);
            rsq[c * n + i] = known[i] ? 0.0 : b[c * n + i] * b[c * n + i];
        }
    wave_adj_host_planes(nV, mt.get(), speed.get(), fac.get());
    wave_born_host_plane(nV, d_cols, fac.get(), d.get(), ldd, fd.get());
    auto b0 = exact<double>(nk);
    for (size_t j = 0; j < nk; j++) b0[j] = b[j];
    wave_born_host(nV, k, d_cols, open ? known.get() : nullptr, fd.get(), e.get(), b.get(), rsq.get());
    bool ok = true;
    int moved = 0;
    for (size_t c = 0; c < kk; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t o = c * n + i;
            const double want = known[i] ? b0[o] : b0[o] + fd[(c % dc) * n + i] * e[o];
            ok = ok && b[o] == want && rsq[o] == (known[i] ? 0.0 : want * want) && std::isfinite(b[o]);
            moved += b[o] != b0[o] ? 1 : 0;
            if (known[i] || (dc > 1 && c % dc == 1)) ok = ok && b[o] == b0[o];   // a known row and the zero column of d leave b as it was
        }
    return ok && moved > 0;
}

int main()
{
    int bad = 0;
    const int sizes[4] = {255, 256, 257, 2100}, shapes[3][2] = {{1, 1}, {3, 1}, {3, 3}};
    for (int nV : sizes)
        for (const auto& s : shapes)
            for (int open = 0; open < 2; open++) {
                const bool ok = run_case(nV, open != 0, s[0], s[1]);
                std::printf("nV %d, %s, k %d, d_cols %d: ok %d\n", nV, open ? "open and clamped" : "closed and free", s[0], s[1], ok ? 1 : 0);
                bad += ok ? 0 : 1;
            }
    return bad;
}
