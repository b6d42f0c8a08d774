"""CPU: the numpy restatement of the V-cycle pieces (tests/f32_reference.py) against the C oracle.

At dtype = float64 the restatement must give the oracle's bits for A, restrict, prolong, the lexicographic Gauss-Seidel sweep, damped Jacobi
and the Chebyshev polynomial: that proves its order of operations without a GPU.  At float32 -- the arithmetic the GPU tests compare the
mixed-precision cycle with (tests/test_gpu_f32_cycle.py) -- every product-sum stays within gamma_32(w_i) sum_j |a_ij| |x_j| of the same sum
in float64 on the same (fp32-rounded) operands."""
import numpy as np
import pytest
import scipy.sparse as sp

import f32_reference as R
from oracle import mesh_np as M
from problems import random_spd_hierarchy, subdiv_problem


def _subdiv(oracle_mod, kind, n_sub):
    p = subdiv_problem(kind=kind, k=1, n_sub=n_sub)
    orc = oracle_mod.OracleMG(p["Ps"])
    orc.precompute(p["A"], p["known"])
    return orc


def _bunny_decimated(oracle_mod, smg):
    V, F = M.read_smgm("bunny.smgm")
    V = M.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)                  # the library's decimator runs on the host
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    orc = oracle_mod.OracleMG(Ps)
    orc.precompute((-M.cotmatrix(V, F)).tocsr(), M.boundary_loop(F))
    return orc


def _random_hub(oracle_mod, smg):
    A, Ps = random_spd_hierarchy(np.random.default_rng(3), 1500, 3, True)
    assert np.diff(A.indptr).max() > 100                        # a hub row
    orc = oracle_mod.OracleMG(Ps)
    orc.precompute(A)
    return orc


CASES = {"subdiv-mcf": lambda o, s: _subdiv(o, "mcf", 2), "subdiv-poisson-pinned": lambda o, s: _subdiv(o, "poisson", 1),
         "bunny-decimated": _bunny_decimated, "random-hub": _random_hub}


def _csr(M_):
    M_ = sp.csr_matrix(M_)
    M_.sort_indices()
    return M_


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_at_float64_is_the_oracle_bit_for_bit(smg_mod, oracle_mod, case):
    orc = CASES[case](oracle_mod, smg_mod)
    rng = np.random.default_rng(11)
    k = 3
    for lv in range(orc.n_levels - 1):
        A, P, PT = _csr(orc.level_A(lv)), _csr(orc.level_P(lv + 1)), _csr(orc.level_PT(lv + 1))
        n, nc = A.shape[0], P.shape[1]
        x, b, xc = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (nc, k))
        assert np.array_equal(R.spmv(R.Ell(A, np.float64), x), orc.A(lv, x)), (case, lv, "A")
        assert np.array_equal(R.restrict(R.Ell(PT, np.float64), x), orc.restrict(lv, x)), (case, lv, "restrict")
        assert np.array_equal(R.spmv(R.Ell(P, np.float64), xc), orc.prolong(lv, xc)), (case, lv, "prolong")
        assert np.array_equal(R.prolong_add(R.Ell(P, np.float64), x, xc), x + orc.prolong(lv, xc)), (case, lv, "prolong-add")
        assert np.array_equal(R.resid(R.Ell(A, np.float64), b, x), b - orc.A(lv, x)), (case, lv, "resid")
        # the smoothers stream A^T: the reference walks column i of A (src/mg_VCycle.cpp:149-155)
        G = _csr(A.T)
        S = R.GsSchedule(G, np.float64, None)                   # lexicographic
        E = R.Ell(G, np.float64)
        for iters in (1, 3):
            orc.set_smoother(lv, "gs")
            assert np.array_equal(R.gauss_seidel(S, b, x, iters), orc.relax(lv, b, x, iters)), (case, lv, "gs", iters)
            orc.set_smoother(lv, "jacobi", 0.8)
            assert np.array_equal(R.jacobi(E, b, x, iters, 0.8), orc.relax(lv, b, x, iters)), (case, lv, "jacobi", iters)
            orc.set_smoother(lv, "chebyshev", 0.1)
            lam = R.spectral_bound(G)
            assert lam == orc.spectral_bound(lv)
            assert np.array_equal(R.chebyshev(E, b, x, iters, lam, 0.1), orc.relax(lv, b, x, iters)), (case, lv, "chebyshev", iters)
        orc.set_smoother(lv, "gs")


def test_a_sweep_in_colour_blocks_is_the_lexicographic_sweep_of_a_valid_colouring(smg_mod, oracle_mod):
    """GsSchedule with a colour pointer (what the GPU tests pass: the device numbering is colour-major) and without one give the same bits
    when the blocks are independent sets, and batches = colours then; a 3-DOF block structure needs three batches per vertex colour."""
    A = _csr(sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(65, 65)))
    perm = np.concatenate([np.arange(0, 65, 2), np.arange(1, 65, 2)])          # red-black
    Ap = _csr(A[perm][:, perm])
    rng = np.random.default_rng(2)
    b, x = rng.uniform(-1, 1, (65, 2)), rng.uniform(-1, 1, (65, 2))
    S2, S1 = R.GsSchedule(Ap, np.float64, [0, 33, 65]), R.GsSchedule(Ap, np.float64, None)
    assert len(S2.batches) == 2
    assert np.array_equal(R.gauss_seidel(S2, b, x, 2), R.gauss_seidel(S1, b, x, 2))
    orc = oracle_mod.OracleMG([sp.csr_matrix(np.ones((65, 1)))])
    orc.precompute(Ap)
    assert np.array_equal(R.gauss_seidel(S2, b, x, 2), orc.relax(0, b, x, 2))
    K = _csr(sp.kron(Ap, sp.csr_matrix(np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 5.0]]))))
    S3 = R.GsSchedule(K, np.float64, [0, 99, 195])
    assert len(S3.batches) == 6
    b3, x3 = rng.uniform(-1, 1, (195, 1)), rng.uniform(-1, 1, (195, 1))
    assert np.array_equal(R.gauss_seidel(S3, b3, x3, 2), R.gauss_seidel(R.GsSchedule(K, np.float64, None), b3, x3, 2))


@pytest.mark.parametrize("case", sorted(CASES))
def test_float32_product_sums_stay_within_the_componentwise_bound(smg_mod, oracle_mod, case):
    """|fl32(sum_j a_ij x_j) - sum_j a_ij x_j| <= gamma_32(w_i) sum_j |a_ij| |x_j| with the operands rounded to fp32 first and the right-hand
    sum taken in float64 (its own rounding, 2^-53 relative per operation, is 2^-29 of the bound's unit and not accounted for)."""
    orc = CASES[case](oracle_mod, smg_mod)
    rng = np.random.default_rng(12)
    k = 2
    f32 = np.float32
    for lv in range(orc.n_levels - 1):
        A, P, PT = _csr(orc.level_A(lv)), _csr(orc.level_P(lv + 1)), _csr(orc.level_PT(lv + 1))
        n, nc = A.shape[0], P.shape[1]
        x, b, xc = [rng.uniform(-1, 1, s).astype(f32) for s in ((n, k), (n, k), (nc, k))]
        EA, EP, EPT = R.Ell(A, f32), R.Ell(P, f32), R.Ell(PT, f32)
        for name, got, exact, bound in (
                ("A", R.spmv(EA, x), EA.sums64(x), R.product_sum_bound(EA, x)),
                ("restrict", R.restrict(EPT, x), EPT.sums64(x), R.product_sum_bound(EPT, x)),
                ("resid", R.resid(EA, b, x), b.astype(np.float64) - EA.sums64(x), R.product_sum_bound(EA, x, b.astype(np.float64) - EA.sums64(x))),
                ("prolong-add", R.prolong_add(EP, x, xc), x.astype(np.float64) + EP.sums64(xc),
                 R.product_sum_bound(EP, xc, x.astype(np.float64) + EP.sums64(xc)))):
            assert got.dtype == f32
            err = np.abs(got.astype(np.float64) - exact)
            assert (err <= bound).all(), (case, lv, name, float((err / np.maximum(bound, 1e-300)).max()))
            assert err.max() > 0.0, (case, lv, name, "an fp32 sum without any rounding error: was it formed in fp32?")
