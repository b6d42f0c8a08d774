"""Python host mirror of the reference's operator API for the solve path, over the C ABI (include/smg.h).

Reference (HTDerekLiu/surface_multigrid_code) usage pattern, README.md:47-48 / 03_mg_solver/main.cpp:38-75:

    vector<mg_data> mg;   mg_precompute(V, F, ratio, nVCoarsest, dec_type, mg);
    min_quad_with_fixed_mg_precompute(A, known, data, mg, solver);
    min_quad_with_fixed_mg_solve(data, RHS, known_val, z0, solver, tol, maxIter, mg, z, rHis);

Here `mg` is a `Hierarchy` (owning the device-resident std::vector<mg_data>, the min_quad_with_fixed_mg_data and
the coarse solver); output arguments become return values.  Nothing in this module computes on the CPU.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import SMG_DEVICE, SMG_HOST, SolveOptsC


class SmgError(RuntimeError):
    def __init__(self, code, where):
        msg = _lib.load().smg_last_error()
        super().__init__("%s failed (%d): %s" % (where, code, msg.decode() if msg else ""))
        self.code = code


def _chk(rc, where):
    if rc != 0:
        raise SmgError(rc, where)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return (np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32),
            np.ascontiguousarray(M.data, dtype=np.float64))


def _colmajor(X):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return np.asfortranarray(X)


SMOOTHERS = {"gs": 0, "jacobi": 1, "hybrid": 2, "chebyshev": 3, "hybrid_chebyshev": 4, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4}


class SolveOpts:
    """tol / maxIter / pre / post with the reference's defaults (src/min_quad_with_fixed_mg.cpp:63,77,102-103)."""

    def __init__(self, tol=1e-3, max_iter=20, pre=2, post=2, verbosity=0, check_every=0, use_graph=1, precision="f64",
                 smoother="gs", omega=0.8, jacobi_max_rows=100000, cheby_fraction=0.1):
        """smoother: "gs" (the reference's relax(), default) / "jacobi" (damped Jacobi on every level) / "hybrid" (Gauss-Seidel on
        the levels with more than `jacobi_max_rows` unknowns, Jacobi below) / "chebyshev", "hybrid_chebyshev" (the same layouts with
        Chebyshev-accelerated Jacobi: one polynomial of degree iters + 1 per relax(iters), include/smg.h)."""
        prec = {"f64": 0, "fp64": 0, 0: 0, "mixed": 1, 1: 1}[precision]
        self.c = SolveOptsC(tol, max_iter, pre, post, verbosity, check_every, use_graph, prec, SMOOTHERS[smoother], omega,
                            jacobi_max_rows, cheby_fraction)


class Hierarchy:
    """std::vector<mg_data> mg (+ solver data) living in HBM.  Wraps smg_hierarchy*."""

    def __init__(self, n_levels=None, handle=None):
        self.L = _lib.load()
        if handle is None:
            handle = self.L.smg_hierarchy_create(int(n_levels))
            if not handle:
                raise SmgError(-1, "smg_hierarchy_create")
        self.h = C.c_void_p(handle)
        self.n = None
        self.known = None

    def __del__(self):
        try:
            if self.h:
                self.L.smg_hierarchy_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- container
    @property
    def n_levels(self):
        return self.L.smg_hierarchy_levels(self.h)

    def set_prolong(self, lv, P):
        """mg[lv].P_full = mg[lv].P = P, mg[lv].PT = P^T (src/mg_precompute.cpp:71-77)."""
        ptr, col, val = _csr(P)
        _chk(self.L.smg_level_set_prolong(self.h, lv, P.shape[0], P.shape[1], _ip(ptr), _ip(col), _dp(val)),
             "smg_level_set_prolong")

    def set_stream(self, stream_ptr):
        """Use the given HIP stream (int handle, e.g. torch.cuda.current_stream().cuda_stream); None / 0 = the default stream."""
        _chk(self.L.smg_hierarchy_set_stream(self.h, C.c_void_p(stream_ptr or 0)), "smg_hierarchy_set_stream")

    def set_smoother(self, smoother="gs", omega=0.0, jacobi_max_rows=-1, cheby_fraction=0.0):
        """Smoother of vcycle()/relax() and the raw entry points (solve() takes it from its SolveOpts)."""
        _chk(self.L.smg_hierarchy_set_smoother(self.h, SMOOTHERS[smoother], omega, jacobi_max_rows), "smg_hierarchy_set_smoother")
        _chk(self.L.smg_hierarchy_set_chebyshev(self.h, cheby_fraction), "smg_hierarchy_set_chebyshev")

    def spectral_bound(self, lv):
        """Gershgorin bound of D^-1 A on level lv (what the Chebyshev-Jacobi smoother uses)."""
        return self.L.smg_level_spectral_bound(self.h, lv)

    def save(self, path):
        _chk(self.L.smg_hierarchy_save(self.h, path.encode()), "smg_hierarchy_save")

    @classmethod
    def load(cls, path):
        out = C.c_void_p()
        _chk(_lib.load().smg_hierarchy_load(path.encode(), C.byref(out)), "smg_hierarchy_load")
        return cls(handle=out.value)

    @classmethod
    def from_prolongs(cls, Ps):
        H = cls(len(Ps) + 1)
        for l, P in enumerate(Ps, start=1):
            H.set_prolong(l, P)
        return H

    # ---- min_quad_with_fixed_mg_precompute
    def precompute(self, A, known=None):
        ptr, col, val = _csr(A)
        n = A.shape[0]
        if known is None or len(known) == 0:
            rc = self.L.smg_precompute(self.h, n, _ip(ptr), _ip(col), _dp(val), None, 0)
            self.known = None
        else:
            kn = np.ascontiguousarray(known, dtype=np.int32)
            rc = self.L.smg_precompute(self.h, n, _ip(ptr), _ip(col), _dp(val), _ip(kn), len(kn))
            self.known = kn
        _chk(rc, "smg_precompute")
        self.n = n

    def precompute_values_device(self, d_val_ptr):
        """Same sparsity as the last precompute, new values already in HBM (device pointer, caller CSR order)."""
        _chk(self.L.smg_precompute_values_device(self.h, d_val_ptr), "smg_precompute_values_device")

    # ---- min_quad_with_fixed_mg_solve (host blocks)
    def solve(self, RHS, z0, known_val=None, opts=None):
        opts = opts or SolveOpts()
        RHS, z0 = _colmajor(RHS), _colmajor(z0)
        n, k = RHS.shape
        z = np.zeros((n, k), order="F")
        r_his = np.zeros(max(opts.c.max_iter, 1))
        n_his, conv = C.c_int(0), C.c_int(0)
        kv_p, ld_kv = None, 0
        if self.known is not None:
            kv = _colmajor(known_val if known_val is not None else np.zeros((len(self.known), k)))
            kv_p, ld_kv = kv.ctypes.data, kv.shape[0]
        rc = self.L.smg_solve(self.h, RHS.ctypes.data, n, kv_p, ld_kv, z0.ctypes.data, n, k, SMG_HOST,
                              C.byref(opts.c), z.ctypes.data, n, _dp(r_his), C.byref(n_his), C.byref(conv))
        _chk(rc, "smg_solve")
        return bool(conv.value), z, r_his[: n_his.value].copy()

    def solve_pcg(self, RHS, z0, known_val=None, opts=None):
        """The same system solved by conjugate gradients with one V-cycle as the preconditioner (include/smg.h: smg_solve_pcg):
        flexible PCG, one recurrence per column, the history and the break test of solve().  Returns (converged, z, r_his)."""
        opts = opts or SolveOpts()
        RHS, z0 = _colmajor(RHS), _colmajor(z0)
        n, k = RHS.shape
        z = np.zeros((n, k), order="F")
        r_his = np.zeros(max(opts.c.max_iter, 1))
        n_his, conv = C.c_int(0), C.c_int(0)
        kv_p, ld_kv = None, 0
        if self.known is not None:
            kv = _colmajor(known_val if known_val is not None else np.zeros((len(self.known), k)))
            kv_p, ld_kv = kv.ctypes.data, kv.shape[0]
        rc = self.L.smg_solve_pcg(self.h, RHS.ctypes.data, n, kv_p, ld_kv, z0.ctypes.data, n, k, SMG_HOST,
                                  C.byref(opts.c), z.ctypes.data, n, _dp(r_his), C.byref(n_his), C.byref(conv))
        _chk(rc, "smg_solve_pcg")
        return bool(conv.value), z, r_his[: n_his.value].copy()

    def eigs(self, mass, nev, block=0, X0=None, opts=None, seed=0):
        """The nev smallest eigenpairs of A_uu x = lambda M_uu x, M = diag(mass) (include/smg.h: smg_eigs): LOBPCG preconditioned by one
        V-cycle.  mass: n entries in the caller's numbering; X0: n x block start or None (a hash of seed) -- with X0 and block = 0 the block
        is X0's column count (a warm start from a returned X iterates its nev columns); opts: tol (relative residual), max_iter (iterations)
        and the cycle's settings.  Returns (evals, X, res_his, n_converged): X is n x nev, M-orthonormal, zero on the known rows; res_his is
        (rows, nev)."""
        opts = opts or SolveOpts(tol=1e-8, max_iter=200)
        mass = np.ascontiguousarray(mass, dtype=np.float64).ravel()
        n = mass.shape[0]
        x0_p, ld_x0 = None, 0
        if X0 is not None:
            X0 = _colmajor(X0)
            if block == 0:
                block = X0.shape[1]
            if X0.shape != (n, block):       # smg_eigs reads n x block doubles from X0
                raise ValueError("X0 must be %d x %d (n x block), got %s" % (n, block, X0.shape))
            x0_p, ld_x0 = X0.ctypes.data, X0.shape[0]
        evals = np.zeros(nev)
        X = np.zeros((n, nev), order="F")
        res = np.zeros((opts.c.max_iter + 1) * nev)
        n_iter, n_conv = C.c_int(0), C.c_int(0)
        _chk(self.L.smg_eigs(self.h, mass.ctypes.data, nev, block, x0_p, ld_x0, SMG_HOST, C.byref(opts.c), seed, _dp(evals), X.ctypes.data, n,
                             _dp(res), C.byref(n_iter), C.byref(n_conv)), "smg_eigs")
        return evals, X, res[: n_iter.value * nev].reshape(n_iter.value, nev), n_conv.value

    def eigs_device(self, mass_ptr, X_ptr, n, nev, block=0, X0_ptr=None, opts=None, seed=0):
        """eigs on device memory: mass (n doubles), X0 (n x block or None) and X (n x nev) are column-major blocks resident in HBM
        (leading dimension n).  With X0, block must be given: smg_eigs reads n x block doubles from it.  Returns (evals, res_his, n_converged)."""
        if X0_ptr and block == 0:
            raise ValueError("eigs_device: a start block X0 needs an explicit block (its column count)")
        opts = opts or SolveOpts(tol=1e-8, max_iter=200)
        evals = np.zeros(nev)
        res = np.zeros((opts.c.max_iter + 1) * nev)
        n_iter, n_conv = C.c_int(0), C.c_int(0)
        _chk(self.L.smg_eigs(self.h, mass_ptr, nev, block, X0_ptr, n if X0_ptr else 0, SMG_DEVICE, C.byref(opts.c), seed, _dp(evals), X_ptr, n,
                             _dp(res), C.byref(n_iter), C.byref(n_conv)), "smg_eigs")
        return evals, res[: n_iter.value * nev].reshape(n_iter.value, nev), n_conv.value

    def solve_device(self, rhs_ptr, z0_ptr, z_ptr, n, k=1, known_val_ptr=None, ld_kv=0, opts=None):
        """min_quad_with_fixed_mg_solve on column-major blocks already resident in HBM (device pointers, leading dimension n):
        the drop-in call, polling the device-side convergence flag every opts.check_every iterations."""
        opts = opts or SolveOpts()
        r_his = np.zeros(max(opts.c.max_iter, 1))
        n_his, conv = C.c_int(0), C.c_int(0)
        _chk(self.L.smg_solve(self.h, rhs_ptr, n, known_val_ptr, ld_kv, z0_ptr, n, k, SMG_DEVICE, C.byref(opts.c), z_ptr, n,
                              _dp(r_his), C.byref(n_his), C.byref(conv)), "smg_solve")
        return bool(conv.value), r_his[: n_his.value].copy()

    def solve_pcg_device(self, rhs_ptr, z0_ptr, z_ptr, n, k=1, known_val_ptr=None, ld_kv=0, opts=None):
        """solve_pcg on column-major blocks already resident in HBM (device pointers, leading dimension n).  Returns (converged, r_his)."""
        opts = opts or SolveOpts()
        r_his = np.zeros(max(opts.c.max_iter, 1))
        n_his, conv = C.c_int(0), C.c_int(0)
        _chk(self.L.smg_solve_pcg(self.h, rhs_ptr, n, known_val_ptr, ld_kv, z0_ptr, n, k, SMG_DEVICE, C.byref(opts.c), z_ptr, n,
                                  _dp(r_his), C.byref(n_his), C.byref(conv)), "smg_solve_pcg")
        return bool(conv.value), r_his[: n_his.value].copy()

    def solve_sharded(self, rhs_ptr, z0_ptr, z_ptr, n, k_local, reduce, known_val_ptr=None, ld_kv=0, opts=None):
        """smg_solve_sharded: this rank's k_local columns (device pointers, leading dimension n; k_local = 0: no columns, pointers may be
        None), the library runs the whole loop and calls reduce(d_sumsq_ptr, count, hip_stream_ptr) -- which must sum the device doubles
        over the ranks in place, ordered on that stream -- once per loop entry.  Returns (converged, r_his)."""
        from ._lib import REDUCE_FN
        opts = opts or SolveOpts()
        r_his = np.zeros(max(opts.c.max_iter, 1))
        n_his, conv = C.c_int(0), C.c_int(0)
        failure = []

        def _cb(ptr, count, stream, _ctx):
            try:
                reduce(ptr, count, stream)
                return 0
            except BaseException as e:   # an exception must not unwind through the C frames
                failure.append(e)
                return 1
        cb = REDUCE_FN(_cb)
        rc = self.L.smg_solve_sharded(self.h, rhs_ptr, n, known_val_ptr, ld_kv, z0_ptr, n, k_local, SMG_DEVICE, C.byref(opts.c), cb, None,
                                      z_ptr, n, _dp(r_his), C.byref(n_his), C.byref(conv))
        if failure:
            raise failure[0]
        _chk(rc, "smg_solve_sharded")
        return bool(conv.value), r_his[: n_his.value].copy()

    # ---- mg_VCycle.h pieces (host blocks in the level's caller numbering)
    def rows(self, lv):
        return self.L.smg_level_rows(self.h, lv)

    def _rows_checked(self, lv, name, *blocks):
        """the C ABI takes bare pointers: a block of the wrong height would be read / written out of bounds"""
        n = self.rows(lv)
        for b in blocks:
            if b.shape[0] != n:
                raise ValueError("%s: level %d has %d rows, the block has %d (rows() is 0 before smg_precompute)" % (name, lv, n, b.shape[0]))
        return n

    def _piece(self, fn, name, lv, x, nout, nin=None):
        x = _colmajor(x)
        if nin is not None and x.shape[0] != nin:
            raise ValueError("%s: expected a block of %d rows, got %d" % (name, nin, x.shape[0]))
        y = np.zeros((nout, x.shape[1]), order="F")
        _chk(fn(self.h, lv, _dp(x), x.shape[1], _dp(y)), name)
        return y

    def A(self, lv, u):
        return self._piece(self.L.smg_apply_A, "smg_apply_A", lv, u, self.rows(lv), self.rows(lv))

    def restrict(self, lv, x):
        return self._piece(self.L.smg_restrict, "smg_restrict", lv, x, self.rows(lv + 1), self.rows(lv))

    def prolong(self, lv, x):
        return self._piece(self.L.smg_prolong, "smg_prolong", lv, x, self.rows(lv), self.rows(lv + 1))

    def relax(self, lv, B, u, iters):
        B, u = _colmajor(B), _colmajor(u).copy(order="F")
        self._rows_checked(lv, "smg_relax", B, u)
        _chk(self.L.smg_relax(self.h, lv, _dp(B), B.shape[1], iters, _dp(u)), "smg_relax")
        return u

    def coarse_solve(self, B, u):
        B, u = _colmajor(B), _colmajor(u).copy(order="F")
        self._rows_checked(self.n_levels - 1, "smg_coarse_solve", B, u)
        _chk(self.L.smg_coarse_solve(self.h, _dp(B), B.shape[1], _dp(u)), "smg_coarse_solve")
        return u

    def vcycle(self, B, u, lv=0, pre=2, post=2):
        B, u = _colmajor(B), _colmajor(u).copy(order="F")
        self._rows_checked(lv, "smg_vcycle", B, u)
        _chk(self.L.smg_vcycle(self.h, _dp(B), pre, post, lv, _dp(u), B.shape[1]), "smg_vcycle")
        return u

    def residual_norm(self, lv, B, u):
        B, u = _colmajor(B), _colmajor(u)
        self._rows_checked(lv, "smg_residual_norm", B, u)
        out = C.c_double(0)
        _chk(self.L.smg_residual_norm(self.h, lv, _dp(B), _dp(u), B.shape[1], C.byref(out)), "smg_residual_norm")
        return out.value

    # ---- introspection
    def matrix(self, lv, which="A", internal=False):
        w = {"A": 0, "P": 1, "PT": 2, "P_full": 3, "Auk": 4}[which]
        nr, nc, nnz = C.c_int(), C.c_int(), C.c_int()
        _chk(self.L.smg_level_get_matrix(self.h, lv, w, int(internal), C.byref(nr), C.byref(nc), C.byref(nnz),
                                         None, None, None), "smg_level_get_matrix")
        ptr = np.zeros(nr.value + 1, np.int32)
        col = np.zeros(max(nnz.value, 1), np.int32)
        val = np.zeros(max(nnz.value, 1))
        _chk(self.L.smg_level_get_matrix(self.h, lv, w, int(internal), None, None, None, _ip(ptr), _ip(col), _dp(val)),
             "smg_level_get_matrix")
        return sp.csr_matrix((val[: nnz.value], col[: nnz.value], ptr), shape=(nr.value, nc.value))

    def perm(self, lv):
        p = np.zeros(self.rows(lv), np.int32)
        _chk(self.L.smg_level_get_perm(self.h, lv, _ip(p)), "smg_level_get_perm")
        return p

    def colors(self, lv):
        nc = C.c_int()
        _chk(self.L.smg_level_get_colors(self.h, lv, C.byref(nc), None), "smg_level_get_colors")
        cp = np.zeros(nc.value + 1, np.int32)
        _chk(self.L.smg_level_get_colors(self.h, lv, None, _ip(cp)), "smg_level_get_colors")
        return cp

    def Adiag(self, lv):
        d = np.zeros(self.rows(lv))
        _chk(self.L.smg_level_get_Adiag(self.h, lv, _dp(d)), "smg_level_get_Adiag")
        return d

    def unknown(self):
        n = C.c_int()
        _chk(self.L.smg_get_unknown(self.h, C.byref(n), None), "smg_get_unknown")
        u = np.zeros(n.value, np.int32)
        _chk(self.L.smg_get_unknown(self.h, None, _ip(u)), "smg_get_unknown")
        return u

    def sell_stats(self, lv, which="A"):
        st, pd, ns = C.c_long(), C.c_long(), C.c_int()
        _chk(self.L.smg_level_sell_stats(self.h, lv, {"A": 0, "P": 1, "PT": 2}[which], C.byref(st), C.byref(pd),
                                         C.byref(ns)), "smg_level_sell_stats")
        return {"stored": st.value, "padded": pd.value, "n_slices": ns.value}

    def first_colour_rows(self, lv):
        """rows of level lv's first colour the restriction launch of level lv - 1 can update itself (0: not available)"""
        return self.L.smg_level_first_colour_rows(self.h, lv)

    # ---- block-sequential Gauss-Seidel for solves with a multiple of 16 columns (k % 16 == 0, k >= 16)
    def set_block_gs(self, min_rows):
        """levels of at least min_rows rows sweep block-sequentially when k % 16 == 0, k >= 16 (< 0: never)"""
        _chk(self.L.smg_hierarchy_set_block_gs(self.h, int(min_rows)), "smg_hierarchy_set_block_gs")

    def block_gs_order(self, lv, k):
        """None when level lv does not sweep block-sequentially for k columns, else a dict: rows (position -> internal row), blk_ptr,
        color_ptr, rim, fill"""
        nb, nc = C.c_int(), C.c_int()
        rc = self.L.smg_level_get_block_gs_order(self.h, lv, int(k), C.byref(nb), C.byref(nc), None, None, None, None)
        if rc < 0:
            _chk(rc, "smg_level_get_block_gs_order")
        if rc == 0:
            return None
        cp, bp, rows, st = np.zeros(nc.value + 1, np.int32), np.zeros(nb.value + 1, np.int32), np.zeros(self.rows(lv), np.int32), np.zeros(2)
        _chk(min(self.L.smg_level_get_block_gs_order(self.h, lv, int(k), None, None, _ip(cp), _ip(bp), _ip(rows), _dp(st)), 0), "smg_level_get_block_gs_order")
        return {"rows": rows, "blk_ptr": bp, "color_ptr": cp, "rim": st[0], "fill": st[1]}

    # ---- piece-wise Gauss-Seidel on the Galerkin levels of decimated hierarchies (csrc/smg_wgs.hpp)
    def set_wave_gs(self, mode="auto"):
        """auto: levels the colour launches serve badly (> 5 colours or rows of > 12 entries); never; all: every Gauss-Seidel level in range"""
        _chk(self.L.smg_hierarchy_set_wave_gs(self.h, {"auto": -1, "never": 0, "all": 1}[mode]), "smg_hierarchy_set_wave_gs")

    def wave_gs_order(self, lv, k=1):
        """None when level lv does not sweep piece-wise for k columns, else a dict: rows (position -> internal row), piece_ptr, color_ptr, rim,
        phases_mean, phases_max"""
        nb, nc = C.c_int(), C.c_int()
        rc = self.L.smg_level_get_wave_gs_order(self.h, lv, int(k), C.byref(nb), C.byref(nc), None, None, None, None)
        if rc < 0:
            _chk(rc, "smg_level_get_wave_gs_order")
        if rc == 0:
            return None
        cp, bp, rows, st = np.zeros(nc.value + 1, np.int32), np.zeros(nb.value + 1, np.int32), np.zeros(self.rows(lv), np.int32), np.zeros(3)
        _chk(min(self.L.smg_level_get_wave_gs_order(self.h, lv, int(k), None, None, _ip(cp), _ip(bp), _ip(rows), _dp(st)), 0), "smg_level_get_wave_gs_order")
        return {"rows": rows, "piece_ptr": bp, "color_ptr": cp, "rim": st[0], "phases_mean": st[1], "phases_max": int(st[2])}

    def gs_order(self, lv, k=1):
        """position -> internal row of the Gauss-Seidel order relax() uses on level lv with k columns: the piece order where the level sweeps
        piece-wise, the block order where it sweeps block-wise, else the internal numbering itself (one launch per colour / overlapped tiling)"""
        w = self.wave_gs_order(lv, k)
        if w is not None:
            return w["rows"]
        b = self.block_gs_order(lv, k)
        if b is not None:
            return b["rows"]
        return np.arange(self.rows(lv), dtype=np.int32)

    # ---- independent meshes in one handle (csrc/smg_union.cpp)
    @classmethod
    def union(cls, members):
        """one block-diagonal hierarchy over the members' prolongations (smg_hierarchy_create_union); precompute() then takes the block-diagonal system"""
        L = _lib.load()
        arr = (C.c_void_p * len(members))(*[m.h for m in members])
        out = C.c_void_p()
        _chk(L.smg_hierarchy_create_union(arr, len(members), C.byref(out)), "smg_hierarchy_create_union")
        return cls(handle=out.value)

    def union_members(self):
        return self.L.smg_union_members(self.h)

    def union_member_rows(self, member):
        a, b = C.c_int(), C.c_int()
        _chk(self.L.smg_union_member_rows(self.h, member, C.byref(a), C.byref(b)), "smg_union_member_rows")
        return a.value, b.value

    def union_history(self, member, cap=4096):
        """(converged, r_his) of one member's own loop in the last solve"""
        rh, n, cv = np.zeros(cap), C.c_int(), C.c_int()
        _chk(self.L.smg_union_get_history(self.h, member, _dp(rh), cap, C.byref(n), C.byref(cv)), "smg_union_get_history")
        return bool(cv.value), rh[:min(n.value, cap)].copy()

    # ---- coarsest-level solver
    def set_coarse_dense_max(self, n_max):
        """coarsest levels of more than n_max unknowns get a sparse Cholesky factorisation instead of a dense inverse"""
        _chk(self.L.smg_hierarchy_set_coarse_dense_max(self.h, int(n_max)), "smg_hierarchy_set_coarse_dense_max")

    def set_coarse_schur(self, when="refactor", n_min=-1):
        """The Schur-complement coarse solver (block elimination + dense inverse of the separator only) for coarsest levels of n_min (default 2048;
        -1: unchanged) to 65 536 unknowns: 'never', 'always' (from the first precompute on) or 'refactor' (default, the choice by cost: below 6 144
        unknowns from the first value-only re-precompute on -- what a time-stepping caller does --, from 6 144 on and above the dense range at once)."""
        _chk(self.L.smg_hierarchy_set_coarse_schur(self.h, {"never": 0, "always": 1, "refactor": 2}[when], int(n_min)), "smg_hierarchy_set_coarse_schur")

    def set_memory_lean(self, on=True):
        """compact SELL panels instead of the fixed panel pitch: ~0.77 x the device memory, the cycle ~15 % slower, same bits; the next precompute is a full one"""
        _chk(self.L.smg_hierarchy_set_memory_lean(self.h, 1 if on else 0), "smg_hierarchy_set_memory_lean")

    def coarse_solver(self):
        ne = C.c_long()
        kind = self.L.smg_hierarchy_coarse_solver(self.h, C.byref(ne))
        return {"kind": {1: "sparse_cholesky", 2: "schur_complement"}.get(kind, "dense_inverse"), "factor_entries": ne.value}

    # ---- block (3-DOF) variant
    def set_block_mode(self, mode="auto"):
        """'auto' (decide at precompute), 'scalar' (never), 'block' (3 x 3 kernels required)."""
        _chk(self.L.smg_hierarchy_set_block_mode(self.h, {"auto": -1, "scalar": 0, "block": 3}.get(mode, mode)), "smg_hierarchy_set_block_mode")

    def block_size(self):
        return self.L.smg_hierarchy_block_size(self.h)

    def block_stats(self, lv=0):
        nb, ns, nc = C.c_long(), C.c_long(), C.c_int()
        _chk(self.L.smg_level_block_stats(self.h, lv, C.byref(nb), C.byref(ns), C.byref(nc)), "smg_level_block_stats")
        return {"blocks": nb.value, "block_slots": ns.value, "vertex_colors": nc.value}

    def block_image(self, lv=0):
        """The block SELL image of A_lv (host-built twin of what the device holds): dict of slice_row, slice_off, slice_w, col (slots x 64),
        val (slots x 9 x 64)."""
        ns, npc = C.c_int(), C.c_int()
        _chk(self.L.smg_level_get_block_image(self.h, lv, C.byref(ns), C.byref(npc), None, None, None, None, None), "smg_level_get_block_image")
        sr, so, sw = np.zeros(ns.value + 1, np.int32), np.zeros(ns.value + 1, np.int32), np.zeros(ns.value, np.int32)
        col, val = np.zeros(npc.value * 64, np.int32), np.zeros(npc.value * 9 * 64, np.float64)
        _chk(self.L.smg_level_get_block_image(self.h, lv, None, None, _ip(sr), _ip(so), _ip(sw), _ip(col), _dp(val)), "smg_level_get_block_image")
        return {"slice_row": sr, "slice_off": so, "slice_w": sw, "col": col.reshape(-1, 64), "val": val.reshape(-1, 9, 64)}

    def device_bytes(self):
        """what this handle holds in HBM, by purpose: dict name -> bytes (incl. "total")"""
        buf = C.create_string_buffer(1 << 16)
        _chk(self.L.smg_debug_device_bytes(self.h, buf, len(buf)), "smg_debug_device_bytes")
        return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines() if ln.strip()}

    def spmv_bytes(self, lv=0, k=1):
        return self.L.smg_level_spmv_bytes(self.h, lv, k)

    def vcycle_bytes(self, k=1, pre=2, post=2):
        return self.L.smg_vcycle_bytes(self.h, k, pre, post)

    # ---- profc mirror
    def prof_enable(self, on=True):
        _chk(self.L.smg_prof_enable(self.h, int(on)), "smg_prof_enable")

    def prof_reset(self):
        _chk(self.L.smg_prof_reset(self.h), "smg_prof_reset")

    def prof_table(self):
        out = {}
        for i in range(self.L.smg_prof_count(self.h)):
            name = C.create_string_buffer(128)
            cnt, ms = C.c_long(), C.c_double()
            _chk(self.L.smg_prof_get(self.h, i, name, 128, C.byref(cnt), C.byref(ms)), "smg_prof_get")
            out[name.value.decode()] = (cnt.value, ms.value)
        return out

    # ---- device-resident interface (torch tensors / raw device pointers)
    def solve_begin(self, rhs_ptr, ld_rhs, z0_ptr, ld_z0, k, known_val_ptr=None, ld_kv=0, opts=None,
                    memspace=SMG_DEVICE):
        opts = opts or SolveOpts()
        self._opts = opts
        _chk(self.L.smg_solve_begin(self.h, rhs_ptr, ld_rhs, known_val_ptr, ld_kv, z0_ptr, ld_z0, k, memspace,
                                    C.byref(opts.c)), "smg_solve_begin")

    def iter_residual(self, d_sumsq_ptr):
        _chk(self.L.smg_solve_iter_residual(self.h, d_sumsq_ptr), "smg_solve_iter_residual")

    def iter_cycle(self, d_sumsq_ptr):
        _chk(self.L.smg_solve_iter_cycle(self.h, d_sumsq_ptr), "smg_solve_iter_cycle")

    def iter_cycle_speculative(self):
        _chk(self.L.smg_solve_iter_cycle_speculative(self.h), "smg_solve_iter_cycle_speculative")

    def iter_commit(self, d_sumsq_ptr):
        _chk(self.L.smg_solve_iter_commit(self.h, d_sumsq_ptr), "smg_solve_iter_commit")

    def outer_iterations(self, n):
        _chk(self.L.smg_raw_outer_iteration(self.h, n), "smg_raw_outer_iteration")

    def poll(self):
        done, nh = C.c_int(), C.c_int()
        _chk(self.L.smg_solve_poll(self.h, C.byref(done), C.byref(nh)), "smg_solve_poll")
        return bool(done.value), nh.value

    def solve_end(self, z_ptr, ld_z, memspace=SMG_DEVICE, max_iter=None):
        cap = max(max_iter or self._opts.c.max_iter, 1)
        r_his = np.zeros(max(cap, 1024))
        n_his, conv = C.c_int(0), C.c_int(0)
        _chk(self.L.smg_solve_end(self.h, z_ptr, ld_z, memspace, _dp(r_his), C.byref(n_his), C.byref(conv)),
             "smg_solve_end")
        return bool(conv.value), r_his[: n_his.value].copy()

    def raw_spmv(self, lv, mode, x_ptr, b_ptr, y_ptr, k=1):
        _chk(self.L.smg_raw_spmv(self.h, lv, mode, x_ptr, b_ptr, y_ptr, k), "smg_raw_spmv")

    def raw_spmv_f32(self, lv, x_ptr, y_ptr, k=1):
        _chk(self.L.smg_raw_spmv_f32(self.h, lv, x_ptr, y_ptr, k), "smg_raw_spmv_f32")

    def raw_relax(self, lv, b_ptr, u_ptr, k=1, iters=1):
        _chk(self.L.smg_raw_relax(self.h, lv, b_ptr, u_ptr, k, iters), "smg_raw_relax")

    def bench_vcycle(self, lv=0, k=1, pre=2, post=2, reps=50):
        out = C.c_double(0)
        _chk(self.L.smg_bench_vcycle(self.h, lv, k, pre, post, reps, C.byref(out)), "smg_bench_vcycle")
        return out.value

    def bench_relax(self, lv=0, k=1, sweeps=2, reps=50):
        out = C.c_double(0)
        _chk(self.L.smg_bench_relax(self.h, lv, k, sweeps, reps, C.byref(out)), "smg_bench_relax")
        return out.value

    def synchronize(self):
        _chk(self.L.smg_synchronize(self.h), "smg_synchronize")


class _MeshObject:
    """What the objects built on a mesh and a caller's hierarchy share (csrc/smg_mesh_object.hpp): the library, the object of the smg_<name>_*
    entry points (self.o; each class also shows it under the short attribute the C ABI's callers know), teardown, bytes, solver, the options
    pointer and the arrays of a local / global iteration."""

    _prefix = o = None

    def _create(self, hierarchy, V, F, *args):
        """smg_<name>_create(hierarchy, V, nV, F, nF, *args, &out); self.o stays None when anything raises, and __del__ then has nothing to do"""
        self.L = _lib.load()
        V = np.ascontiguousarray(V, dtype=np.float64)
        F = np.ascontiguousarray(F, dtype=np.int32)
        self.n, self.nF = V.shape[0], F.shape[0]
        out = C.c_void_p()
        _chk(self._fn("create")(hierarchy.h, _dp(V), self.n, _ip(F), self.nF, *args, C.byref(out)), self._prefix + "create")
        self.o = C.c_void_p(out.value)

    def _fn(self, name):
        return getattr(self.L, self._prefix + name)

    def _call(self, name, *args):
        _chk(self._fn(name)(self.o, *args), self._prefix + name)

    def __del__(self):
        try:
            if self.o:
                self._fn("destroy")(self.o)
                self.o = None
        except Exception:
            pass

    def set_solver(self, pcg=-1):
        """1: the solves run smg_solve_pcg (default), 0: smg_solve's stationary loop, -1: unchanged."""
        self._call("set_solver", int(pcg))

    def device_bytes(self):
        return self._fn("device_bytes")(self.o)

    @staticmethod
    def _opts(o):
        return C.byref(o.c) if o is not None else None

    def _iterate(self, name, max_iter, *args):
        """smg_<name>(o, *args, energy_his, cycles, &n_iter) -> (E_0 .. E_n_iter, the loop entries of each inner solve)"""
        E = np.zeros(max_iter + 1)
        cyc = np.zeros(max(max_iter, 1), dtype=np.int32)
        nit = C.c_int(0)
        self._call(name, *args, _dp(E), _ip(cyc), C.byref(nit))
        return E[:nit.value + 1].copy(), cyc[:nit.value].copy()


class HeatGeodesics(_MeshObject):
    """Geodesic distance by the heat method on the V-cycle (include/smg.h: smg_geodesics_*), libigl's heat_geodesics_precompute / _solve.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  t: None (or 0) for
    the default (bounding-box diagonal / 12)^2, else the heat step's time.  voronoi: the mass matrix of the heat step."""

    _prefix = "smg_geodesics_"
    g = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, t=None, voronoi=False):
        self._create(hierarchy, V, F, float(t or 0.0), int(bool(voronoi)))
        self.cycles = (0, 0)

    @property
    def t(self):
        return self.L.smg_geodesics_time(self.g)

    def set_solver(self, heat_pcg=-1, poisson_pcg=-1):
        """1: solve the stage by smg_solve_pcg (default), 0: by smg_solve's stationary loop, -1: unchanged."""
        self._call("set_solver", int(heat_pcg), int(poisson_pcg))

    @staticmethod
    def _sources(sources):
        """an int, or a list whose entries are ints or index lists -> (k, src_ptr, src)"""
        if isinstance(sources, (int, np.integer)):
            sources = [[int(sources)]]
        sets = [[int(s)] if isinstance(s, (int, np.integer)) else [int(x) for x in s] for s in sources]
        ptr = np.zeros(len(sets) + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([len(s) for s in sets])
        src = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in sets]) if sets else np.zeros(0), dtype=np.int32)
        return len(sets), ptr, src

    def _solve(self, k, ptr, src, memspace, heat_opts, poisson_opts, D_ptr, ld_d):
        cyc = (C.c_int * 2)()
        self._call("solve", k, _ip(ptr), _ip(src) if len(src) else None, memspace, self._opts(heat_opts), self._opts(poisson_opts), D_ptr, ld_d, cyc)
        self.cycles = (cyc[0], cyc[1])
        return self.cycles

    def distance(self, sources, heat_opts=None, poisson_opts=None):
        """Distances to each source set: sources = an int (one set of one vertex) or a list of sets (an int or a list of vertex indices
        each).  Returns the n x k array, column c = the distance to set c; self.cycles = the loop entries of the two solves."""
        k, ptr, src = self._sources(sources)
        D = np.zeros((self.n, max(k, 1)), order="F")
        self._solve(k, ptr, src, SMG_HOST, heat_opts, poisson_opts, D.ctypes.data, self.n)
        return D

    def distance_device(self, sources, D_ptr, ld_d=None, heat_opts=None, poisson_opts=None):
        """distance() into a column-major n x k block resident in HBM (device pointer, leading dimension ld_d, default n).  Returns the
        loop entries of the two solves."""
        return self._solve(*self._sources(sources), SMG_DEVICE, heat_opts, poisson_opts, D_ptr, ld_d or self.n)


class ArapDeformer(_MeshObject):
    """As-rigid-as-possible deformation on the V-cycle (include/smg.h: smg_arap_*), libigl's arap_precompute / arap_solve (spokes energy).

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  V: the rest pose,
    handles: the vertices whose positions deform() is given; the system -L of the rest pose is precomputed here, once."""

    _prefix = "smg_arap_"
    a = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, handles):
        self.handles = np.ascontiguousarray(handles, dtype=np.int32).reshape(-1)
        self._create(hierarchy, V, F, _ip(self.handles), self.handles.shape[0])

    def _run(self, hp_ptr, ld_hp, U0_ptr, ld_u0, memspace, max_iter, rel_tol, opts, U_ptr, ld_u):
        return self._iterate("solve", max_iter, hp_ptr, ld_hp, U0_ptr, ld_u0, memspace, int(max_iter), float(rel_tol), self._opts(opts), U_ptr, ld_u)

    def deform(self, handle_pos, U0=None, max_iter=10, rel_tol=0.0, opts=None):
        """handle_pos: n_handles x 3 (row r = the position of handles[r]); U0: the n x 3 start, None = the rest pose.  Returns
        (U, energy_his, cycles): the n x 3 positions after the iterations run, E_0 .. E_n_iter, the loop entries of each inner solve."""
        hp = _colmajor(handle_pos)
        assert hp.shape == (self.handles.shape[0], 3)
        U0 = None if U0 is None else _colmajor(U0)
        assert U0 is None or U0.shape == (self.n, 3)
        U = np.zeros((self.n, 3), order="F")
        E, cyc = self._run(hp.ctypes.data, hp.shape[0], U0.ctypes.data if U0 is not None else None, self.n, SMG_HOST, max_iter, rel_tol, opts,
                           U.ctypes.data, self.n)
        return U, E, cyc

    def deform_device(self, hp_ptr, U_ptr, ld_u=None, U0_ptr=None, ld_u0=None, ld_hp=None, max_iter=10, rel_tol=0.0, opts=None):
        """deform() between column-major blocks resident in HBM (device pointers; leading dimensions default to n_handles and n).
        Returns (energy_his, cycles)."""
        return self._run(hp_ptr, ld_hp or self.handles.shape[0], U0_ptr, ld_u0 or self.n, SMG_DEVICE, max_iter, rel_tol, opts, U_ptr, ld_u or self.n)


class Parameterizer(_MeshObject):
    """Harmonic and as-rigid-as-possible flattening of a disk mesh on the V-cycle (include/smg.h: smg_param_*): the cotangent-weight harmonic
    map to the circle of the mesh's area, and the local / global iteration of Liu et al. 2008 from it.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F), a disk (one boundary loop, Euler characteristic 1); its prolongations are
    copied, it is not modified.  The system -L is precomputed here, twice: with the boundary loop known and with its first vertex known."""

    STATS = ("flipped", "max_aspect", "mean_aspect", "mean_area_ratio", "symmetric_dirichlet", "area")
    _prefix = "smg_param_"
    p = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F):
        self._create(hierarchy, V, F)
        self.cycles = 0

    def boundary(self):
        """the boundary loop, in order; its first vertex is the one the global step pins"""
        n = C.c_int(0)
        self._call("boundary", C.byref(n), None)
        loop = np.zeros(n.value, dtype=np.int32)
        self._call("boundary", None, _ip(loop))
        return loop

    def harmonic_device(self, UV_ptr, ld_uv=None, opts=None, memspace=SMG_DEVICE):
        """harmonic() into a column-major n x 2 block resident in HBM (device pointer).  Returns the loop entries of the solve."""
        cyc = C.c_int(0)
        self._call("harmonic", memspace, self._opts(opts), UV_ptr, ld_uv or self.n, C.byref(cyc))
        self.cycles = cyc.value
        return self.cycles

    def harmonic(self, opts=None):
        """The n x 2 harmonic map to the circle; self.cycles = the loop entries of the solve."""
        UV = np.zeros((self.n, 2), order="F")
        self.harmonic_device(UV.ctypes.data, self.n, opts, SMG_HOST)
        return UV

    def flatten_device(self, UV_ptr, ld_uv=None, UV0_ptr=None, ld_uv0=None, max_iter=10, rel_tol=0.0, opts=None, memspace=SMG_DEVICE):
        """flatten() between column-major n x 2 blocks resident in HBM (device pointers; leading dimensions default to n).  Returns
        (energy_his, cycles)."""
        return self._iterate("arap", max_iter, UV0_ptr, ld_uv0 or self.n, memspace, int(max_iter), float(rel_tol), self._opts(opts), UV_ptr, ld_uv or self.n)

    def flatten(self, UV0=None, max_iter=10, rel_tol=0.0, opts=None):
        """ARAP flattening from UV0 (n x 2; None = the harmonic map).  Returns (UV, energy_his, cycles): the map after the iterations run,
        E_0 .. E_n_iter, the loop entries of each inner solve."""
        UV0 = None if UV0 is None else _colmajor(UV0)
        assert UV0 is None or UV0.shape == (self.n, 2)
        UV = np.zeros((self.n, 2), order="F")
        E, cyc = self.flatten_device(UV.ctypes.data, self.n, UV0.ctypes.data if UV0 is not None else None, self.n, max_iter, rel_tol, opts, SMG_HOST)
        return UV, E, cyc

    def distortion(self, UV):
        """(sigma, stats): sigma nF x 2 (the singular values of every face's Jacobian, larger first) and the dict of STATS."""
        UV = _colmajor(UV)
        assert UV.shape == (self.n, 2)
        sigma = np.zeros((self.nF, 2), order="F")
        st = np.zeros(6)
        self._call("distortion", UV.ctypes.data, self.n, SMG_HOST, sigma.ctypes.data, _dp(st))
        stats = dict(zip(self.STATS, st.tolist()))
        stats["flipped"] = int(stats["flipped"])
        return sigma, stats


class MembraneSim(_MeshObject):
    """Implicit-Euler steps of a pressurised membrane on the block V-cycle (include/smg.h: smg_membrane_*), the time step of the
    reference's 06_example_balloon_sim.  material: "neo_hookean" (default), "stvk" or "tension_field" (or 0, 1, 2).

    hierarchy: a block Hierarchy (mg_precompute_block) whose level 0 is the mesh (V, F) with 3 DOFs per vertex; its prolongations are copied, it
    is not modified.  V: the rest pose.  params: the fields of smg_membrane_params (young, poisson, thickness, mass_scale, dt, pressure,
    newton_iters, ls_c, ls_shrink, ls_min_alpha, eig_floor, eig_value); the state starts as (V, 0)."""

    MATERIALS = ("neo_hookean", "stvk", "tension_field")
    _prefix = "smg_membrane_"
    m = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, material="neo_hookean", **params):
        self.params = membrane_params(**params)
        mat = self._material_id(material)
        self._create(hierarchy, V, F, C.byref(self.params))
        if mat != 0:
            self.set_material(mat)

    @classmethod
    def _material_id(cls, material):
        if isinstance(material, str):
            if material not in cls.MATERIALS:
                raise ValueError("unknown membrane material %r (one of %s)" % (material, ", ".join(cls.MATERIALS)))
            return cls.MATERIALS.index(material)
        return int(material)

    def set_material(self, material):
        """material: "neo_hookean" / 0, "stvk" / 1, "tension_field" / 2; legal between any two steps, the state is kept."""
        self._call("set_material", self._material_id(material))

    @property
    def material(self):
        return self.MATERIALS[self.L.smg_membrane_material(self.m)]

    def set_solver(self, pcg=-1):
        """0: smg_solve's stationary loop (default, the reference), 1: smg_solve_pcg, -1: unchanged."""
        self._call("set_solver", int(pcg))

    def set_state(self, pos=None, qdot=None):
        """pos, qdot: n x 3 (None: the rest pose / zero)"""
        pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64).reshape(self.n, 3)
        qdot = None if qdot is None else np.ascontiguousarray(qdot, dtype=np.float64).reshape(self.n, 3)
        self._call("set_state", None if pos is None else pos.ctypes.data, None if qdot is None else qdot.ctypes.data, SMG_HOST)

    def set_state_device(self, pos_ptr, qdot_ptr):
        """the same from n x 3 row-major blocks resident in HBM (device pointers; 0 / None as above)"""
        self._call("set_state", pos_ptr or None, qdot_ptr or None, SMG_DEVICE)

    def state(self):
        """(pos, qdot), n x 3 each"""
        pos, qdot = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        self._call("get_state", pos.ctypes.data, qdot.ctypes.data, SMG_HOST)
        return pos, qdot

    def step(self, opts=None):
        """One time step.  Returns a dict: objective (f(qdot) before every Newton iteration and after the last), alpha (the accepted steps, 0 where
        the line search gave up), cycles (the loop entries of every solve)."""
        n_it = self.params.newton_iters
        obj, alpha = np.zeros(n_it + 1), np.zeros(max(n_it, 1))
        cyc = np.zeros(max(n_it, 1), dtype=np.int32)
        done = C.c_int(0)
        self._call("step", self._opts(opts), _dp(obj), _dp(alpha), _ip(cyc), C.byref(done))
        return {"objective": obj, "alpha": alpha[:n_it].copy(), "cycles": cyc[:n_it].copy()}


class ProjectiveDynamics(_MeshObject):
    """Projective-dynamics steps of a membrane with triangle-strain constraints on the scalar V-cycle (include/smg.h: smg_pd_*; Bouaziz et al.
    2014).  The global matrix (density / dt^2) M0 - stiffness L is precomputed here, once; a step is a handful of 3-column warm-started solves.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  V: the rest pose.
    pins: the vertices a step holds at given positions (none is legal).  params: the fields of smg_pd_params (dt, density, stiffness,
    sigma_min, sigma_max, pressure, gravity); the state starts as (V, 0)."""

    STATS = ("max_sigma1", "min_sigma2", "outside_band", "mean_distance2")
    _prefix = "smg_pd_"
    d = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, pins=(), **params):
        self.params = pd_params(**params)
        self.pins = np.ascontiguousarray(pins, dtype=np.int32).reshape(-1)
        self._create(hierarchy, V, F, _ip(self.pins) if self.pins.size else None, self.pins.shape[0], C.byref(self.params))

    def set_state(self, pos=None, vel=None):
        """pos, vel: n x 3 (None keeps)"""
        pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64).reshape(self.n, 3)
        vel = None if vel is None else np.ascontiguousarray(vel, dtype=np.float64).reshape(self.n, 3)
        self._call("set_state", None if pos is None else pos.ctypes.data, None if vel is None else vel.ctypes.data, SMG_HOST)

    def set_state_device(self, pos_ptr, vel_ptr):
        """the same from n x 3 row-major blocks resident in HBM (device pointers; 0 / None keeps)"""
        self._call("set_state", pos_ptr or None, vel_ptr or None, SMG_DEVICE)

    def state(self):
        """(pos, vel), n x 3 each"""
        pos, vel = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        self._call("get_state", pos.ctypes.data, vel.ctypes.data, SMG_HOST)
        return pos, vel

    def state_device(self, pos_ptr, vel_ptr):
        """state() into n x 3 row-major blocks resident in HBM (device pointers; 0 / None skips)"""
        self._call("get_state", pos_ptr or None, vel_ptr or None, SMG_DEVICE)

    def set_forces(self, pressure, gravity=None):
        """legal between any two steps; gravity: 3 numbers, None keeps"""
        g = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64).reshape(3)
        self._call("set_forces", float(pressure), None if g is None else _dp(g))

    def set_strain_limits(self, sigma_min, sigma_max):
        """legal between any two steps; (1, 1) is the ARAP membrane"""
        self._call("set_strain_limits", float(sigma_min), float(sigma_max))

    def step(self, pin_pos=None, max_iter=10, rel_tol=0.0, opts=None):
        """One time step.  pin_pos: n_pins x 3, the pins at the end of the step (None keeps them).  Returns (energy_his, cycles): E_0 .. E_n_iter
        and the loop entries of each inner solve."""
        hp = None if pin_pos is None else np.ascontiguousarray(pin_pos, dtype=np.float64).reshape(self.pins.shape[0], 3)
        return self._iterate("step", max_iter, None if hp is None else hp.ctypes.data, SMG_HOST, int(max_iter), float(rel_tol), self._opts(opts))

    def step_device(self, pin_pos_ptr=None, max_iter=10, rel_tol=0.0, opts=None):
        """step() with the pin positions (n_pins x 3 xyz rows) resident in HBM (device pointer; 0 / None keeps)"""
        return self._iterate("step", max_iter, pin_pos_ptr or None, SMG_DEVICE, int(max_iter), float(rel_tol), self._opts(opts))

    def strain(self):
        """(sigma, stats) of the current state: sigma nF x 2 (the singular values of every face's deformation gradient, larger first) and the
        dict of STATS."""
        sigma = np.zeros((self.nF, 2), order="F")
        st = np.zeros(4)
        self._call("strain", SMG_HOST, sigma.ctypes.data, _dp(st))
        stats = dict(zip(self.STATS, st.tolist()))
        stats["outside_band"] = int(stats["outside_band"])
        return sigma, stats


class Denoiser(_MeshObject):
    """Feature-preserving denoising of a triangle mesh on the scalar V-cycle (include/smg.h: smg_denoise_*): the bilateral normal filter of
    Zheng et al. 2011 over the faces that share a vertex, then positions that follow the filtered normals.  The global matrix fidelity M - L
    is precomputed here, once; an update is a handful of 3-column warm-started solves.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  V: the noisy positions.
    params: the fields of smg_denoise_params (sigma_s, sigma_r, fidelity, normal_iters); sigma_s <= 0 selects the mean centroid distance of
    the neighbourhoods.  fidelity has units 1 / length^2: normalise the mesh to unit area first."""

    _prefix = "smg_denoise_"
    d = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, **params):
        self.params = denoise_params(**params)
        self._create(hierarchy, V, F, C.byref(self.params))

    @property
    def sigma_s(self):
        """the value in use"""
        return self.L.smg_denoise_sigma_s(self.d)

    def set_filter(self, sigma_s=0.0, sigma_r=0.0, normal_iters=-1):
        """legal between any two calls; sigma_s <= 0, sigma_r <= 0 or normal_iters < 0 keeps the current value"""
        self._call("set_filter", float(sigma_s), float(sigma_r), int(normal_iters))

    def filter(self, normals=None):
        """The filter from normals (nF x 3; None: the input mesh's own); the result (nF x 3) is returned and latched for update()."""
        m0 = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64).reshape(self.nF, 3)
        out = np.zeros((self.nF, 3))
        self._call("filter", None if m0 is None else m0.ctypes.data, SMG_HOST, out.ctypes.data)
        return out

    def filter_device(self, normals_ptr=None, out_ptr=None):
        """filter() between nF x 3 row-major blocks resident in HBM (device pointers; 0 / None: the mesh's normals / no output)"""
        self._call("filter", normals_ptr or None, SMG_DEVICE, out_ptr or None)

    def update(self, X0=None, max_iter=10, rel_tol=0.0, opts=None):
        """The vertex update against the latched normals from X0 (n x 3; None: V).  Returns (X, energy_his, cycles)."""
        X0 = None if X0 is None else np.ascontiguousarray(X0, dtype=np.float64).reshape(self.n, 3)
        X = np.zeros((self.n, 3))
        E, cyc = self._iterate("update", max_iter, None if X0 is None else X0.ctypes.data, SMG_HOST, int(max_iter), float(rel_tol), self._opts(opts),
                               X.ctypes.data)
        return X, E, cyc

    def update_device(self, X_ptr, X0_ptr=None, max_iter=10, rel_tol=0.0, opts=None):
        """update() between n x 3 row-major blocks resident in HBM (device pointers).  Returns (energy_his, cycles)."""
        return self._iterate("update", max_iter, X0_ptr or None, SMG_DEVICE, int(max_iter), float(rel_tol), self._opts(opts), X_ptr)

    def run(self, max_iter=10, rel_tol=0.0, opts=None):
        """filter(), then update() from V, in one call.  Returns (X, energy_his, cycles)."""
        X = np.zeros((self.n, 3))
        E, cyc = self._iterate("run", max_iter, SMG_HOST, int(max_iter), float(rel_tol), self._opts(opts), X.ctypes.data)
        return X, E, cyc

    def run_device(self, X_ptr, max_iter=10, rel_tol=0.0, opts=None):
        """run() into an n x 3 row-major block resident in HBM (device pointer).  Returns (energy_his, cycles)."""
        return self._iterate("run", max_iter, SMG_DEVICE, int(max_iter), float(rel_tol), self._opts(opts), X_ptr)


class Stylizer(_MeshObject):
    """Cubic and normal-driven stylization on the scalar V-cycle (include/smg.h: smg_stylize_*; Liu and Jacobson 2019 and 2021): as-rigid-as-possible
    deformation with the penalty lambda a_i |Q R_i n_i|_1 (cubic) or lambda a_i |R_i n_i - t_i|^2 (normal-driven, after set_targets) on every
    vertex's rotated normal.  The global matrix -L is smg_arap's and is precomputed here, once; the local step is an ADMM loop per vertex.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  V: the rest pose; bring it
    to a unit bounding box first: lambda is tuned at that scale.  pins: the vertices whose positions run() is given (None: vertex 0).
    params: the fields of smg_stylize_params (lambda_, rho0, abs_tol, rel_tol, mu, tau, admm_iters)."""

    _prefix = "smg_stylize_"
    s = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, pins=None, **params):
        self.pins = np.ascontiguousarray([0] if pins is None else pins, dtype=np.int32).reshape(-1)
        self.params = stylize_params(**params)
        self._create(hierarchy, V, F, _ip(self.pins), self.pins.shape[0], C.byref(self.params))

    def set_params(self, **params):
        """legal between calls, nothing is rebuilt; fields not named keep their values"""
        p = stylize_params(**{**{k: getattr(self.params, k) for k, _ in self.params._fields_}, **params})
        self._call("set_params", C.byref(p))
        self.params = p

    def set_lambda(self, lam=None):
        """per-vertex weights (n values, finite and >= 0); None: back to the uniform lambda"""
        lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64).reshape(self.n)
        self._call("set_lambda", None if lam is None else _dp(lam))

    def set_frame(self, Q=None):
        """Q: the 3 x 3 rotation whose rows are the cube's axes; None: the identity"""
        Q = None if Q is None else np.ascontiguousarray(Q, dtype=np.float64).reshape(9)
        self._call("set_frame", None if Q is None else _dp(Q))

    def set_targets(self, targets=None):
        """n x 3 unit target normals select the normal-driven mode; None selects the cubic mode"""
        T = None if targets is None else np.ascontiguousarray(targets, dtype=np.float64).reshape(self.n, 3)
        self._call("set_targets", None if T is None else _dp(T))

    def normals(self):
        """(n_i as n x 3, a_i): the unit area-weighted vertex normals and the barycentric vertex areas of the rest pose"""
        nrm, area = np.zeros((self.n, 3)), np.zeros(self.n)
        self._call("normals", _dp(nrm), _dp(area))
        return nrm, area

    def admm_stats(self):
        """the ADMM iteration counts of the last local step: dict(min, mean, max, at_cap, iters)"""
        lo, hi, cap, mean = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        it = np.zeros(self.n, dtype=np.int32)
        self._call("admm_stats", C.byref(lo), C.byref(mean), C.byref(hi), C.byref(cap), _ip(it))
        return dict(min=lo.value, mean=mean.value, max=hi.value, at_cap=cap.value, iters=it)

    def _run(self, pp_ptr, ld_pp, U0_ptr, ld_u0, memspace, max_iter, rel_tol, opts, U_ptr, ld_u):
        return self._iterate("run", max_iter, pp_ptr, ld_pp, U0_ptr, ld_u0, memspace, int(max_iter), float(rel_tol), self._opts(opts), U_ptr, ld_u)

    def run(self, pin_pos=None, U0=None, max_iter=10, rel_tol=0.0, opts=None):
        """pin_pos: n_pins x 3 (row r = the position of pins[r]; None: the rest positions); U0: the n x 3 start, None = the rest pose.  Returns
        (U, energy_his, cycles): the n x 3 positions after the iterations run, E_0 .. E_n_iter, the loop entries of each inner solve."""
        pp = None if pin_pos is None else _colmajor(pin_pos)
        assert pp is None or pp.shape == (self.pins.shape[0], 3)
        U0 = None if U0 is None else _colmajor(U0)
        assert U0 is None or U0.shape == (self.n, 3)
        U = np.zeros((self.n, 3), order="F")
        E, cyc = self._run(None if pp is None else pp.ctypes.data, self.pins.shape[0], None if U0 is None else U0.ctypes.data, self.n, SMG_HOST,
                           max_iter, rel_tol, opts, U.ctypes.data, self.n)
        return U, E, cyc

    def run_device(self, U_ptr, pp_ptr=None, ld_u=None, U0_ptr=None, ld_u0=None, ld_pp=None, max_iter=10, rel_tol=0.0, opts=None):
        """run() between column-major blocks resident in HBM (device pointers; leading dimensions default to n_pins and n).
        Returns (energy_his, cycles)."""
        return self._run(pp_ptr or None, ld_pp or self.pins.shape[0], U0_ptr or None, ld_u0 or self.n, SMG_DEVICE, max_iter, rel_tol, opts, U_ptr,
                         ld_u or self.n)


class Morpher(_MeshObject):
    """Gradient-domain morphing on the scalar V-cycle (include/smg.h: smg_morph_*): Poisson reconstruction from per-face gradients, pose
    interpolation through the faces' polar factors and deformation transfer.  k sets are 3k right-hand sides of one constant matrix, -L of the
    rest pose with the pinned rows known, precomputed here, once: every query is one 3k-column solve.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  V: the rest pose.
    pins: the vertices whose positions a query is given, or takes from its default (None: vertex 0)."""

    _prefix = "smg_morph_"
    m = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, pins=None):
        self.pins = np.ascontiguousarray([0] if pins is None else pins, dtype=np.int32).reshape(-1)
        self._create(hierarchy, V, F, _ip(self.pins), self.pins.shape[0])

    def _tail(self, k, pin_pos, U0, opts):
        """the arguments the three queries share, for host blocks: pin_pos k x n_pins x 3 and U0 k x n x 3, or None = the query's defaults"""
        nh = self.pins.shape[0]
        pp = None if pin_pos is None else np.asfortranarray(np.asarray(pin_pos, dtype=np.float64).reshape(k, nh, 3).transpose(1, 0, 2).reshape(nh, 3 * k))
        u0 = None if U0 is None else np.asfortranarray(np.asarray(U0, dtype=np.float64).reshape(k, self.n, 3).transpose(1, 0, 2).reshape(self.n, 3 * k))
        U = np.zeros((self.n, 3 * k), order="F")
        cyc = C.c_int(0)
        keep = (pp, u0)
        return keep, U, cyc, (None if pp is None else pp.ctypes.data, nh, None if u0 is None else u0.ctypes.data, self.n, SMG_HOST, self._opts(opts),
                              U.ctypes.data, self.n, C.byref(cyc))

    def _sets(self, U, k):
        return np.ascontiguousarray(U.reshape(self.n, k, 3).transpose(1, 0, 2))

    def reconstruct(self, J, pin_pos=None, U0=None, opts=None):
        """J: k x nF x 3 x 3 (or nF x 3 x 3) per-face gradients.  pin_pos: k x n_pins x 3 (None: the pins' rest positions); U0: k x n x 3 (None: the
        rest pose).  Returns (U as k x n x 3, the loop entries of the solve)."""
        J = np.ascontiguousarray(J, dtype=np.float64).reshape(-1, self.nF, 9)
        k = J.shape[0]
        keep, U, cyc, tail = self._tail(k, pin_pos, U0, opts)
        self._call("reconstruct", J.ctypes.data, k, *tail)
        return self._sets(U, k), cyc.value

    def interpolate(self, X, ts, pin_pos=None, U0=None, opts=None):
        """X: the n x 3 pose; ts: the k times (0: the rest pose, 1: X; any finite value).  pin_pos None: the pins blended linearly; U0 None: the
        linear blend of the rest pose and X.  Returns (U as k x n x 3, the loop entries of the solve)."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(self.n, 3)
        t = np.ascontiguousarray(np.atleast_1d(ts), dtype=np.float64).reshape(-1)
        k = t.shape[0]
        keep, U, cyc, tail = self._tail(k, pin_pos, U0, opts)
        self._call("interpolate", X.ctypes.data, _dp(t), k, *tail)
        return self._sets(U, k), cyc.value

    def transfer(self, S0, S1s, Fs=None, pin_pos=None, U0=None, opts=None):
        """S0: the source's rest pose (nVs x 3), S1s: its k poses (k x nVs x 3 or nVs x 3), Fs: its faces (nF x 3, face f corresponds to face f of
        this mesh; None: this mesh's faces).  Returns (U as k x n x 3, the loop entries of the solve)."""
        S0 = np.ascontiguousarray(S0, dtype=np.float64).reshape(-1, 3)
        S1 = np.ascontiguousarray(S1s, dtype=np.float64).reshape(-1, S0.shape[0], 3)
        Fs = None if Fs is None else np.ascontiguousarray(Fs, dtype=np.int32).reshape(self.nF, 3)
        k = S1.shape[0]
        keep, U, cyc, tail = self._tail(k, pin_pos, U0, opts)
        self._call("transfer", S0.ctypes.data, S0.shape[0], None if Fs is None else _ip(Fs), S1.ctypes.data, k, *tail)
        return self._sets(U, k), cyc.value

    def _device_tail(self, U_ptr, ld_u, pp_ptr, ld_pp, U0_ptr, ld_u0, opts, cyc):
        return (pp_ptr or None, ld_pp or self.pins.shape[0], U0_ptr or None, ld_u0 or self.n, SMG_DEVICE, self._opts(opts), U_ptr, ld_u or self.n,
                C.byref(cyc))

    def reconstruct_device(self, J_ptr, k, U_ptr, ld_u=None, pp_ptr=None, ld_pp=None, U0_ptr=None, ld_u0=None, opts=None):
        """reconstruct() between blocks resident in HBM (device pointers; J: k sets of nF x 9; U, U0: n x 3k and pin_pos: n_pins x 3k column-major,
        leading dimensions default to n and n_pins).  Returns the loop entries of the solve."""
        cyc = C.c_int(0)
        self._call("reconstruct", J_ptr, int(k), *self._device_tail(U_ptr, ld_u, pp_ptr, ld_pp, U0_ptr, ld_u0, opts, cyc))
        return cyc.value

    def interpolate_device(self, X_ptr, ts, U_ptr, ld_u=None, pp_ptr=None, ld_pp=None, U0_ptr=None, ld_u0=None, opts=None):
        """interpolate() with the pose (n x 3 xyz rows) and the blocks resident in HBM; ts stays on the host."""
        t = np.ascontiguousarray(np.atleast_1d(ts), dtype=np.float64).reshape(-1)
        cyc = C.c_int(0)
        self._call("interpolate", X_ptr, _dp(t), t.shape[0], *self._device_tail(U_ptr, ld_u, pp_ptr, ld_pp, U0_ptr, ld_u0, opts, cyc))
        return cyc.value

    def transfer_device(self, S0_ptr, nVs, S1_ptr, k, U_ptr, Fs=None, ld_u=None, pp_ptr=None, ld_pp=None, U0_ptr=None, ld_u0=None, opts=None):
        """transfer() with the source's rest pose (nVs x 3) and poses (k x nVs x 3) and the blocks resident in HBM; Fs stays on the host."""
        Fs = None if Fs is None else np.ascontiguousarray(Fs, dtype=np.int32).reshape(self.nF, 3)
        cyc = C.c_int(0)
        self._call("transfer", S0_ptr, int(nVs), None if Fs is None else _ip(Fs), S1_ptr, int(k),
                   *self._device_tail(U_ptr, ld_u, pp_ptr, ld_pp, U0_ptr, ld_u0, opts, cyc))
        return cyc.value


class MeanCurvatureFlow(_MeshObject):
    """Conformalized mean-curvature flow on the scalar V-cycle (include/smg.h: smg_flow_*; Kazhdan, Solomon, Ben-Chen 2012; the reference's
    05_example_mean_curvature_flow) and, on a closed genus-0 mesh, the conformal map to the sphere it converges to.  L of the rest mesh is
    assembled once; a step rebuilds the barycentric mass of the current positions, re-precomputes M - delta L by values and runs one warm-started
    3-column solve.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  delta: the time step on
    the unit-area mesh.  normalize: normalize_unit_area on the rest mesh and after every step.  stop_sphericity > 0 ends step() early."""

    STATS = ("mean_ratio", "max_ratio", "flipped", "sphericity")
    _prefix = "smg_flow_"
    f = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, delta=0.01, normalize=True, stop_sphericity=0.0):
        self.params = flow_params(delta=delta, normalize=int(normalize), stop_sphericity=stop_sphericity)
        self._create(hierarchy, V, F, C.byref(self.params))

    def set_params(self, **params):
        """delta, stop_sphericity: the following steps use them (normalize is fixed at create)"""
        p = _lib.FlowParamsC(self.params.delta, self.params.normalize, self.params.stop_sphericity)
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError("unknown flow parameter %r" % k)
            setattr(p, k, int(v) if k == "normalize" else v)
        self._call("set_params", C.byref(p))
        self.params = p

    def step(self, n=1, opts=None):
        """n steps.  Returns (sphericity_his, cycles) trimmed to the steps done: the sphericity before every step and after the last one, and the
        loop entries of each solve."""
        his = np.zeros(n + 1)
        cyc = np.zeros(max(n, 1), dtype=np.int32)
        done = C.c_int(0)
        self._call("step", int(n), self._opts(opts), _dp(his), _ip(cyc), C.byref(done))
        return his[:done.value + 1].copy(), cyc[:done.value].copy()

    def positions(self):
        """the state, n x 3"""
        U = np.zeros((self.n, 3), order="F")
        self._call("positions", SMG_HOST, U.ctypes.data, self.n)
        return np.ascontiguousarray(U)

    def positions_device(self, U_ptr, ld_u=None):
        """the state into an n x 3 column-major block resident in HBM (device pointer)"""
        self._call("positions", SMG_DEVICE, U_ptr, ld_u or self.n)

    def set_positions(self, U):
        U = np.asfortranarray(np.asarray(U, dtype=np.float64).reshape(self.n, 3))
        self._call("set_positions", U.ctypes.data, self.n, SMG_HOST)

    def set_positions_device(self, U_ptr, ld_u=None):
        self._call("set_positions", U_ptr, ld_u or self.n, SMG_DEVICE)

    def reset(self):
        """back to the (normalised) rest mesh"""
        self._call("reset")

    def sphere(self):
        """(S, sigma, stats) of the current state: S n x 3 on the unit sphere, sigma nF x 2 (the singular values of the Jacobian rest face ->
        sphere face, larger first) and the dict of STATS.  Needs a closed genus-0 mesh."""
        S = np.zeros((self.n, 3), order="F")
        sigma = np.zeros((self.nF, 2), order="F")
        st = np.zeros(4)
        self._call("sphere", SMG_HOST, S.ctypes.data, self.n, sigma.ctypes.data, _dp(st))
        stats = dict(zip(self.STATS, st.tolist()))
        stats["flipped"] = int(stats["flipped"])
        return np.ascontiguousarray(S), sigma, stats


class HodgeDecomposition(_MeshObject):
    """Helmholtz-Hodge decomposition of per-face tangent vector fields with vertex potentials (include/smg.h: smg_hodge_*; Tong, Lombeyda,
    Hirani, Desbrun 2003): Xt = grad u + J grad v + H.  k fields are 2k right-hand sides of -L: ONE 2k-column solve on a closed mesh, two
    k-column solves on a mesh with boundary.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified."""

    ENERGY = ("field", "gradient", "rotation", "remainder")
    _prefix = "smg_hodge_"
    g = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F):
        self._create(hierarchy, V, F)

    @property
    def is_closed(self):
        """whether the mesh has no boundary edge"""
        return bool(self._fn("is_closed")(self.o))

    def decompose(self, X, parts=False, opts=None):
        """X: nF x 3 or k x nF x 3.  Returns (u, v, energy, cycles), or with parts (u, v, parts, energy, cycles): u, v n x k; parts k x nF x 3 x 3
        (G, R, H of every face); energy k x 4 (sum A |Xt|^2, |G|^2, |R|^2, |H|^2); cycles: the loop entries of the u solve and of the v solve."""
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1, self.nF, 3))
        k = X.shape[0]
        u, v = np.zeros((self.n, k), order="F"), np.zeros((self.n, k), order="F")
        P = np.zeros((k, self.nF, 3, 3)) if parts else None
        E = np.zeros((k, 4))
        cyc = np.zeros(2, dtype=np.int32)
        self._call("decompose", X.ctypes.data, k, SMG_HOST, self._opts(opts), u.ctypes.data, self.n, v.ctypes.data, self.n,
                   P.ctypes.data if parts else None, _dp(E), _ip(cyc))
        return (u, v, P, E, cyc) if parts else (u, v, E, cyc)

    def field(self, u, v):
        """X = grad u + J grad v: k x nF x 3 for n x k potentials (nF x 3 for vectors)"""
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        single = u.ndim == 1
        u, v = np.asfortranarray(u.reshape(self.n, -1)), np.asfortranarray(v.reshape(self.n, -1))
        k = u.shape[1]
        X = np.zeros((k, self.nF, 3))
        self._call("field", u.ctypes.data, self.n, v.ctypes.data, self.n, k, SMG_HOST, X.ctypes.data)
        return X[0] if single else X


class ConformalMetric(_MeshObject):
    """Discrete conformal metrics with prescribed angle sums (include/smg.h: smg_conformal_*; Springborn, Schroeder, Pinkall 2008): one log scale
    factor u per vertex so that the metric l exp((u_i + u_j) / 2) has the angle sum Theta at every free vertex.  Newton's method on the convex
    energy; every step re-precomputes the cotangent matrix of the current metric by values and runs one 1-column solve.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  fixed: the vertices whose
    u is given (at least one), in the order solve() takes their values."""

    _prefix = "smg_conformal_"
    c = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, fixed, **params):
        self.fixed = np.ascontiguousarray(fixed, dtype=np.int32).reshape(-1)
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.params = conformal_params(**params)
        self._create(hierarchy, V, F, _ip(self.fixed), self.fixed.shape[0], C.byref(self.params))

    def set_params(self, **params):
        """grad_tol, max_newton, inner_rel_tol of the following calls"""
        p = _lib.ConformalParamsC(self.params.grad_tol, self.params.max_newton, self.params.inner_rel_tol)
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError("unknown conformal parameter %r" % k)
            setattr(p, k, v)
        self._call("set_params", C.byref(p))
        self.params = p

    def solve(self, Theta, u_fixed=None, opts=None):
        """Newton from the current u.  Theta: n target angle sums; u_fixed: the fixed vertices' u (None: zeros).  Returns (grad_his, step_his,
        cycles, converged): max |g| of every iterate, the accepted step lengths and the loop entries of the solves, trimmed to the steps done."""
        Theta = np.ascontiguousarray(Theta, dtype=np.float64).reshape(self.n)
        uf = None if u_fixed is None else np.ascontiguousarray(u_fixed, dtype=np.float64).reshape(self.fixed.shape[0])
        cap = self.params.max_newton
        g, st, cyc = np.zeros(cap + 1), np.zeros(max(cap, 1)), np.zeros(max(cap, 1), dtype=np.int32)
        nn, conv = C.c_int(0), C.c_int(0)
        self._call("solve", Theta.ctypes.data, None if uf is None else uf.ctypes.data, SMG_HOST, self._opts(opts), _dp(g), _dp(st), _ip(cyc),
                   C.byref(nn), C.byref(conv))
        return g[:nn.value + 1].copy(), st[:nn.value].copy(), cyc[:nn.value].copy(), bool(conv.value)

    def solve_device(self, Theta_ptr, u_fixed_ptr=None, opts=None):
        """solve() with Theta (and u_fixed) resident in HBM (device pointers)"""
        cap = self.params.max_newton
        g, st, cyc = np.zeros(cap + 1), np.zeros(max(cap, 1)), np.zeros(max(cap, 1), dtype=np.int32)
        nn, conv = C.c_int(0), C.c_int(0)
        self._call("solve", Theta_ptr, u_fixed_ptr or None, SMG_DEVICE, self._opts(opts), _dp(g), _dp(st), _ip(cyc), C.byref(nn), C.byref(conv))
        return g[:nn.value + 1].copy(), st[:nn.value].copy(), cyc[:nn.value].copy(), bool(conv.value)

    def reset(self):
        """u = 0"""
        self._call("reset")

    def u(self):
        u = np.zeros(self.n)
        self._call("u", SMG_HOST, u.ctypes.data)
        return u

    def u_device(self, u_ptr):
        self._call("u", SMG_DEVICE, u_ptr)

    def set_u(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.n)
        self._call("set_u", u.ctypes.data, SMG_HOST)

    def set_u_device(self, u_ptr):
        self._call("set_u", u_ptr, SMG_DEVICE)

    def angle_sums(self):
        """the achieved angle sums of the current u at all n vertices"""
        a = np.zeros(self.n)
        self._call("angle_sums", SMG_HOST, a.ctypes.data)
        return a

    def lengths(self):
        """nF x 3: the current length of the edge opposite every corner"""
        lt = np.zeros((self.nF, 3))
        self._call("lengths", SMG_HOST, lt.ctypes.data)
        return lt

    def stats(self):
        """the broken faces of the last accepted iterate and their maximum over the last solve"""
        s = np.zeros(2)
        self._call("stats", _dp(s))
        return dict(broken=int(s[0]), broken_max=int(s[1]))

    def layout(self):
        """(X n x 2, stats) of mesh.unfold on the current lengths: meaningful for a flat metric on a disk"""
        from . import mesh
        return mesh.unfold(self.F, self.lengths(), self.n)


def conformal_params(**params):
    """smg_conformal_params with the library's defaults and the given fields"""
    p = _lib.load().smg_conformal_params_default()
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown conformal parameter %r" % k)
        setattr(p, k, v)
    return p


class EmdResult:
    """upper, lower, gap = (upper - lower) / upper (0 where upper is 0) and residual per column; iterations; potential (n x k) and flow
    (k x nF x 3) where asked for, else None"""

    def __init__(self, upper, lower, iterations, residual, potential, flow):
        self.upper, self.lower, self.iterations, self.residual, self.potential, self.flow = upper, lower, iterations, residual, potential, flow
        with np.errstate(divide="ignore", invalid="ignore"):
            self.gap = np.where(upper > 0.0, (upper - lower) / np.where(upper > 0.0, upper, 1.0), 0.0)

    def __repr__(self):
        return "EmdResult(upper=%r, lower=%r, iterations=%d)" % (self.upper, self.lower, self.iterations)


class EarthMover(_MeshObject):
    """Earth mover's (1-Wasserstein) distances between distributions on a mesh with geodesic ground cost, with the transport flow and the
    Kantorovich potential (include/smg.h: smg_emd_*; Solomon, Rustamov, Guibas, Butscher 2014).  ADMM on the Beckmann form: every iteration is ONE
    warm-started k-column solve of -L for k pairs of distributions, one vertex kernel and one face kernel; the stopping rule is a certificate,
    lower <= the discrete optimum <= upper (up to the solve's residual).

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  params: gap_tol,
    max_iter, check_every, alpha, rho_scale, inner_rel_tol."""

    _prefix = "smg_emd_"
    e = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, **params):
        self.params = emd_params(**params)
        self.V, self.F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
        self._create(hierarchy, V, F, C.byref(self.params))

    def set_params(self, **params):
        """gap_tol, max_iter, check_every, alpha, rho_scale, inner_rel_tol of the following calls"""
        p = _lib.EmdParamsC(*[getattr(self.params, f) for f, _ in _lib.EmdParamsC._fields_])
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError("unknown earth mover parameter %r" % k)
            setattr(p, k, v)
        self._call("set_params", C.byref(p))
        self.params = p

    def masses(self, density):
        """integrated masses per vertex of a per-vertex density (n or n x k): the barycentric mass matrix times the density"""
        from . import mesh
        return mesh.massmatrix(self.V, self.F, "barycentric") @ np.asarray(density, dtype=np.float64)

    def distance(self, mu0, mu1, warm=False, potential=False, flow=False, opts=None):
        """mu0, mu1: integrated masses per vertex, n or n x k, with equal sums per column.  Returns an EmdResult."""
        mu0 = np.asfortranarray(np.asarray(mu0, dtype=np.float64).reshape(self.n, -1))
        mu1 = np.asfortranarray(np.asarray(mu1, dtype=np.float64).reshape(self.n, -1))
        k = mu0.shape[1]
        if mu1.shape[1] != k:
            raise ValueError("mu0 and mu1 differ in their columns")
        up, lo, res = np.zeros(k), np.zeros(k), np.zeros(k)
        P = np.zeros((self.n, k), order="F") if potential else None
        J = np.zeros((k, self.nF, 3)) if flow else None
        nit = C.c_int(0)
        self._call("solve", mu0.ctypes.data, self.n, mu1.ctypes.data, self.n, k, SMG_HOST, self._opts(opts), int(bool(warm)), _dp(up), _dp(lo),
                   C.byref(nit), _dp(res), P.ctypes.data if potential else None, self.n, J.ctypes.data if flow else None)
        return EmdResult(up, lo, nit.value, res, P, J)

    def distance_device(self, mu0_ptr, ld0, mu1_ptr, ld1, k, warm=False, potential_ptr=None, ld_p=0, flow_ptr=None, opts=None):
        """distance() with the masses (and the optional outputs) resident in HBM (device pointers, column-major with leading dimensions)"""
        up, lo, res = np.zeros(k), np.zeros(k), np.zeros(k)
        nit = C.c_int(0)
        self._call("solve", mu0_ptr, ld0, mu1_ptr, ld1, k, SMG_DEVICE, self._opts(opts), int(bool(warm)), _dp(up), _dp(lo), C.byref(nit), _dp(res),
                   potential_ptr or None, ld_p or self.n, flow_ptr or None)
        return EmdResult(up, lo, nit.value, res, None, None)


def emd_params(**params):
    """smg_emd_params with the library's defaults and the given fields"""
    p = _lib.load().smg_emd_params_default()
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown earth mover parameter %r" % k)
        setattr(p, k, v)
    return p


class SurfaceFluid(_MeshObject):
    """Incompressible flow on a surface in vorticity - stream-function form (include/smg.h: smg_fluid_*): (-L) psi = -m (w - wbar),
    u = n x grad psi, a finite-volume transport of w on the barycentric dual cells, SSP Runge-Kutta stages, optional implicit viscosity.  The
    state w (n x k: k independent simulations) lives on the device; every stage is ONE warm-started k-column solve of -L and one vertex kernel.
    On a mesh with boundary psi = 0 there (the boundary is a streamline); the viscous solve has the natural boundary condition for w, not a
    no-slip wall.

    hierarchy: a scalar Hierarchy whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.  params: theta, stages,
    viscosity, dt, cfl."""

    _prefix = "smg_fluid_"
    f = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, **params):
        self.params = fluid_params(**params)
        self.k = 0
        self._create(hierarchy, V, F, C.byref(self.params))

    @property
    def closed(self):
        return bool(self.L.smg_fluid_is_closed(self.o))

    def set_params(self, **params):
        """theta, stages, viscosity, dt, cfl of the following steps; zero and non-zero viscosity cannot change"""
        p = _lib.FluidParamsC(*[getattr(self.params, f) for f, _ in _lib.FluidParamsC._fields_])
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError("unknown fluid parameter %r" % k)
            setattr(p, k, v)
        self._call("set_params", C.byref(p))
        self.params = p

    def set_vorticity(self, w):
        """w: n or n x k; sets k, zeroes psi and the times"""
        w = np.asfortranarray(np.asarray(w, dtype=np.float64).reshape(self.n, -1))
        self._call("set_vorticity", w.ctypes.data, self.n, w.shape[1], SMG_HOST)
        self.k = w.shape[1]

    def set_vorticity_device(self, w_ptr, ld, k):
        self._call("set_vorticity", w_ptr, ld, k, SMG_DEVICE)
        self.k = k

    def step(self, n_steps=1, opts=None):
        """n_steps steps -> (cfl n_done x k, time n_done x k, cycles n_done): every step's cfl, the time after it, the loop entries of its solves"""
        k = max(self.k, 1)
        cfl, time, cyc = np.zeros((max(n_steps, 1), k)), np.zeros((max(n_steps, 1), k)), np.zeros(max(n_steps, 1), dtype=np.int32)
        nd = C.c_int(0)
        try:
            self._call("step", int(n_steps), self._opts(opts), _dp(cfl), _dp(time), _ip(cyc), C.byref(nd))
        finally:
            self.n_done = nd.value
        return cfl[:nd.value].copy(), time[:nd.value].copy(), cyc[:nd.value].copy()

    def vorticity(self):
        w = np.zeros((self.n, max(self.k, 1)), order="F")
        self._call("vorticity", w.ctypes.data, self.n, SMG_HOST)
        return w

    def vorticity_device(self, w_ptr, ld):
        self._call("vorticity", w_ptr, ld, SMG_DEVICE)

    def stream(self, opts=None):
        """psi (n x k) of the current state"""
        psi = np.zeros((self.n, max(self.k, 1)), order="F")
        self._call("stream", self._opts(opts), psi.ctypes.data, self.n, SMG_HOST)
        return psi

    def velocity(self, opts=None):
        """U (k x nF x 3) = n x grad psi of the current state"""
        U = np.zeros((max(self.k, 1), self.nF, 3))
        self._call("velocity", self._opts(opts), U.ctypes.data, SMG_HOST)
        return U

    def diagnostics(self, opts=None):
        """dict(circulation, enstrophy, energy, wbar), k each"""
        d = np.zeros((4, max(self.k, 1)))
        self._call("diagnostics", self._opts(opts), _dp(d))
        return dict(circulation=d[0].copy(), enstrophy=d[1].copy(), energy=d[2].copy(), wbar=d[3].copy())


def fluid_params(**params):
    """smg_fluid_params with the library's defaults and the given fields"""
    p = _lib.load().smg_fluid_params_default()
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown fluid parameter %r" % k)
        setattr(p, k, v)
    return p


class ReactionDiffusion(_MeshObject):
    """Two-species reaction-diffusion on a surface (include/smg.h: smg_rd_*): per column u_t = Du Laplace u + R_u(u, v), v_t = Dv Laplace v +
    R_v(u, v) with the no-flux boundary condition, R_u and R_v bivariate cubics given per column as 20 coefficients (reactions.py has the named
    models).  The reaction is explicit (react_substeps Euler sub-steps in one vertex kernel), the diffusion implicit on the constant matrices
    M + dt D (-L): two k-column solves, ONE 2k-column solve when Du == Dv, one k-column solve when Dv == 0.  The state (n x k each: k independent
    simulations) lives on the device.

    hierarchy: a scalar Hierarchy of at least two levels whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified."""

    _prefix = "smg_rd_"
    g = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, Du, Dv, dt, react_substeps=1, stop_change=0.0):
        self.params = rd_params(Du=Du, Dv=Dv, dt=dt, react_substeps=react_substeps, stop_change=stop_change)
        self.k = 0
        self._create(hierarchy, V, F, C.byref(self.params))

    def set_params(self, **params):
        """Du, Dv, dt, react_substeps, stop_change of the following steps; a changed dt Du or dt Dv re-precomputes by values; the case of
        handle use (Du != Dv with Dv > 0 | Du == Dv | Dv == 0) cannot change"""
        p = _lib.RdParamsC(*[getattr(self.params, f) for f, _ in _lib.RdParamsC._fields_])
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError("unknown reaction-diffusion parameter %r" % k)
            setattr(p, k, v)
        self._call("set_params", C.byref(p))
        self.params = p

    def set_state(self, u, v, coeff):
        """u, v: n or n x k; coeff: 20 (every column's reaction) or k x 20; sets k"""
        u = np.asfortranarray(np.asarray(u, dtype=np.float64).reshape(self.n, -1))
        v = np.asfortranarray(np.asarray(v, dtype=np.float64).reshape(self.n, -1))
        k = u.shape[1]
        if v.shape[1] != k:
            raise ValueError("u has %d columns, v has %d" % (k, v.shape[1]))
        coeff = np.asarray(coeff, dtype=np.float64)
        coeff = np.ascontiguousarray(np.broadcast_to(coeff, (k, 20)) if coeff.ndim == 1 else coeff.reshape(k, 20))
        self._call("set_state", u.ctypes.data, v.ctypes.data, self.n, k, _dp(coeff), SMG_HOST)
        self.k = k

    def set_state_device(self, u_ptr, v_ptr, ld, k, coeff):
        coeff = np.ascontiguousarray(np.asarray(coeff, dtype=np.float64).reshape(k, 20))
        self._call("set_state", u_ptr, v_ptr, ld, k, _dp(coeff), SMG_DEVICE)
        self.k = k

    def step(self, n_steps=1, opts=None):
        """at most n_steps steps -> (mass n_done x 2k: sum m u then sum m v per column, change n_done x k, cycles n_done x 2: the loop entries of
        the step's solves); self.n_done: the steps done"""
        k, rows = max(self.k, 1), max(n_steps, 1)
        mass, change, cyc = np.zeros((rows, 2 * k)), np.zeros((rows, k)), np.zeros((rows, 2), dtype=np.int32)
        nd = C.c_int(0)
        try:
            self._call("step", int(n_steps), self._opts(opts), _dp(mass), _dp(change), _ip(cyc), C.byref(nd))
        finally:
            self.n_done = nd.value
        return mass[:nd.value].copy(), change[:nd.value].copy(), cyc[:nd.value].copy()

    def state(self):
        """(u, v), n x k each"""
        u, v = np.zeros((self.n, max(self.k, 1)), order="F"), np.zeros((self.n, max(self.k, 1)), order="F")
        self._call("state", u.ctypes.data, v.ctypes.data, self.n, SMG_HOST)
        return u, v

    def state_device(self, u_ptr, v_ptr, ld):
        self._call("state", u_ptr, v_ptr, ld, SMG_DEVICE)


def rd_params(**params):
    """smg_rd_params with the library's defaults and the given fields"""
    p = _lib.load().smg_rd_params_default()
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown reaction-diffusion parameter %r" % k)
        setattr(p, k, v)
    return p


class WaveEquation(_MeshObject):
    """The wave equation on a surface with shots and receivers (include/smg.h: smg_wave_*): per column Mt u_tt + Sigma Mt u_t + C u = f(t) with
    C = -L, Mt = diag(m / speed^2) and Sigma = diag(sigma), stepped by the trapezoidal rule in (u, v = u_t): ONE k-column solve of the constant
    matrix diag((1 + sigma dt / 2) mt) + (dt^2 / 4) C per step, k experiments at once.  clamped=False is the free boundary; clamped=True holds
    the boundary vertices at 0.  The state (n x k each) lives on the device.

    hierarchy: a scalar Hierarchy of at least two levels whose level 0 is the mesh (V, F); its prolongations are copied, it is not modified.
    speed, sigma: n values or None (1 everywhere; `damping` everywhere)."""

    _prefix = "smg_wave_"
    g = property(lambda self: self.o)

    def __init__(self, hierarchy, V, F, dt, speed=None, sigma=None, damping=0.0, clamped=False):
        self.params = wave_params(dt=dt, damping=damping, clamped=int(clamped))
        self.k = self.n_src = self.n_rec = self.lin_steps = 0
        n = np.asarray(V).shape[0]
        speed = None if speed is None else np.ascontiguousarray(np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,)))
        sigma = None if sigma is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,)))
        self._create(hierarchy, V, F, None if speed is None else _dp(speed), None if sigma is None else _dp(sigma), C.byref(self.params))

    def set_params(self, **params):
        """dt, damping of the following steps: a changed value re-precomputes by values; clamped cannot change"""
        p = _lib.WaveParamsC(*[getattr(self.params, f) for f, _ in _lib.WaveParamsC._fields_])
        for k, v in params.items():
            if k not in dict(p._fields_):
                raise TypeError("unknown wave parameter %r" % k)
            setattr(p, k, v)
        self._call("set_params", C.byref(p))
        self.params = p

    def set_state(self, u, v):
        """u, v: n or n x k; sets k"""
        u = np.asfortranarray(np.asarray(u, dtype=np.float64).reshape(self.n, -1))
        v = np.asfortranarray(np.asarray(v, dtype=np.float64).reshape(self.n, -1))
        k = u.shape[1]
        if v.shape[1] != k:
            raise ValueError("u has %d columns, v has %d" % (k, v.shape[1]))
        self.k = 0
        self._call("set_state", u.ctypes.data, v.ctypes.data, self.n, k, SMG_HOST)
        self.k = k

    def set_state_device(self, u_ptr, v_ptr, ld, k):
        self.k = 0
        self._call("set_state", u_ptr, v_ptr, ld, k, SMG_DEVICE)
        self.k = k

    def set_sources(self, idx):
        """the vertices that step()'s signal drives: no vertex twice, none on a clamped boundary"""
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
        self._call("set_sources", _ip(idx), idx.size)
        self.n_src = idx.size

    def set_receivers(self, idx):
        """the vertices whose u every step records"""
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
        self._call("set_receivers", _ip(idx), idx.size)
        self.n_rec = idx.size

    def step(self, n_steps=1, signal=None, energy=True, opts=None):
        """at most n_steps steps -> (energy n_done x 2k: kinetic then potential per column, or None; traces n_done x n_rec x k; cycles n_done);
        signal: (n_steps + 1) x n_src x k nodal forces at the step times, or None; self.n_done: the steps done"""
        k, rows = max(self.k, 1), max(n_steps, 1)
        E = np.zeros((rows, 2 * k)) if energy else None
        tr, cyc = np.zeros((rows, self.n_rec, k)), np.zeros(rows, dtype=np.int32)
        if signal is not None:
            signal = np.ascontiguousarray(np.asarray(signal, dtype=np.float64))
            if signal.size != (rows + 1) * self.n_src * k:
                raise ValueError("the signal has %d entries, (n_steps + 1) x n_src x k = %d are needed" % (signal.size, (rows + 1) * self.n_src * k))
        nd = C.c_int(0)
        try:
            self._call("step", int(n_steps), None if signal is None else _dp(signal), self._opts(opts), None if E is None else _dp(E),
                       _dp(tr) if self.n_rec else None, _ip(cyc), C.byref(nd))
        finally:
            self.n_done = nd.value
        return None if E is None else E[:nd.value].copy(), tr[:nd.value].copy(), cyc[:nd.value].copy()

    def state(self):
        """(u, v), n x k each"""
        u, v = np.zeros((self.n, max(self.k, 1)), order="F"), np.zeros((self.n, max(self.k, 1)), order="F")
        self._call("state", u.ctypes.data, v.ctypes.data, self.n, SMG_HOST)
        return u, v

    def state_device(self, u_ptr, v_ptr, ld):
        self._call("state", u_ptr, v_ptr, ld, SMG_DEVICE)

    def set_speed(self, speed):
        """a new speed for the following steps (n values, a scalar, or None: 1 everywhere): a value-only re-precompute; the state is kept"""
        speed = None if speed is None else np.ascontiguousarray(np.broadcast_to(np.asarray(speed, dtype=np.float64), (self.n,)))
        self._call("set_speed", None if speed is None else _dp(speed))

    def gradient(self, n_steps, signal=None, observed=None, speed=True, state=True, grad_signal=None, opts=None):
        """n_steps steps from the current state, then the adjoint pass: the misfit J_c = 0.5 sum (traces - observed)^2 per column and its exact
        discrete gradients -> WaveGradient.  signal: as step(); observed: n_steps x n_rec x k or None (zeros); speed, state: whether grad_speed and
        (grad_u0, grad_v0) are wanted; grad_signal: whether the signal's gradient is (None: where a signal is given).  With none of them wanted
        the backward pass is skipped.  The state afterwards is the one n_steps steps on; self.n_done: the forward steps done"""
        k, rows = max(self.k, 1), max(n_steps, 1)
        want_gs = (signal is not None) if grad_signal is None else bool(grad_signal)
        if signal is not None:
            signal = np.ascontiguousarray(np.asarray(signal, dtype=np.float64))
            if signal.size != (rows + 1) * self.n_src * k:
                raise ValueError("the signal has %d entries, (n_steps + 1) x n_src x k = %d are needed" % (signal.size, (rows + 1) * self.n_src * k))
        if observed is not None:
            observed = np.ascontiguousarray(np.asarray(observed, dtype=np.float64))
            if observed.size != rows * self.n_rec * k:
                raise ValueError("observed has %d entries, n_steps x n_rec x k = %d are needed" % (observed.size, rows * self.n_rec * k))
        r = WaveGradient()
        r.misfit = np.zeros(k)
        r.grad_speed = np.zeros((self.n, k), order="F") if speed else None
        r.grad_u0, r.grad_v0 = (np.zeros((self.n, k), order="F"), np.zeros((self.n, k), order="F")) if state else (None, None)
        r.grad_signal = np.zeros((rows + 1, self.n_src, k)) if want_gs else None
        r.traces, r.cycles = np.zeros((rows, self.n_rec, k)), np.zeros(2 * rows, dtype=np.int32)
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        nd = C.c_int(0)
        try:
            self._call("gradient", int(n_steps), ptr(signal), ptr(observed), self._opts(opts), _dp(r.misfit), ptr(r.grad_speed), self.n, ptr(r.grad_u0),
                       ptr(r.grad_v0), self.n, ptr(r.grad_signal), _dp(r.traces) if self.n_rec else None, _ip(r.cycles), C.byref(nd))
        finally:
            self.n_done = nd.value
        if speed or state or want_gs:
            self.lin_steps = rows   # the shape of gauss_newton()'s traces; whether the point stands is the library's to say
        return r

    def gauss_newton(self, d, product=True, traces=False, opts=None):
        """Born traces J d and the Gauss-Newton product H d = J' J d at the run of the last gradient() call that asked for a gradient (include/smg.h:
        smg_wave_gauss_newton) -> WaveGaussNewton.  d: n values or n x k, a speed perturbation (one direction for every shot, or one per shot);
        product: whether H d is wanted (False: Born modelling alone, the backward pass is skipped); traces: whether born_traces is.  The curvature
        |J d|^2 per column always is.  The state is not touched"""
        k, rows = max(self.k, 1), max(self.lin_steps, 1)
        d = np.asfortranarray(np.asarray(d, dtype=np.float64).reshape(self.n, -1))
        r = WaveGaussNewton()
        r.product = np.zeros((self.n, k), order="F") if product else None
        r.born_traces = np.zeros((rows, self.n_rec, k)) if traces else None
        r.curvature, r.cycles = np.zeros(k), np.zeros(2 * rows if product else rows, dtype=np.int32)
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        self._call("gauss_newton", ptr(d), self.n, d.shape[1], self._opts(opts), ptr(r.product), self.n, ptr(r.born_traces), _dp(r.curvature), _ip(r.cycles))
        return r


class WaveGradient:
    """what WaveEquation.gradient returns: misfit (k), grad_speed, grad_u0, grad_v0 (n x k, one gradient per shot), grad_signal ((n_steps + 1) x
    n_src x k), traces (n_steps x n_rec x k), cycles (2 n_steps: the forward solves, then the backward solves in the order they ran); a gradient
    that was not asked for is None"""
    misfit = grad_speed = grad_u0 = grad_v0 = grad_signal = traces = cycles = None


class WaveGaussNewton:
    """what WaveEquation.gauss_newton returns: product (n x k, one H d per shot; None where it was not asked for), born_traces (n_steps x n_rec x
    k, or None), curvature (k: |J d|^2 per column), cycles (the tangent solves, then the backward solves in the order they ran)"""
    product = born_traces = curvature = cycles = None


def wave_params(**params):
    """smg_wave_params with the library's defaults and the given fields"""
    p = _lib.load().smg_wave_params_default()
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown wave parameter %r" % k)
        setattr(p, k, v)
    return p


def flow_params(**params):
    """smg_flow_params with the library's defaults and the given fields"""
    p = _lib.load().smg_flow_params_default()
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown flow parameter %r" % k)
        setattr(p, k, v)
    return p


def stylize_params(**params):
    """smg_stylize_params with the library's defaults and the given fields (lambda is spelled lambda_)"""
    p = _lib.StylizeParamsC()
    _lib.load().smg_stylize_params_default(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown stylization parameter %r" % k)
        setattr(p, k, v)
    return p


def denoise_params(**params):
    """smg_denoise_params with the library's defaults and the given fields"""
    p = _lib.DenoiseParamsC()
    _lib.load().smg_denoise_params_default(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown denoising parameter %r" % k)
        setattr(p, k, v)
    return p


def pd_params(**params):
    """smg_pd_params with the library's defaults and the given fields (gravity: 3 numbers)"""
    p = _lib.PdParamsC()
    _lib.load().smg_pd_params_default(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown projective-dynamics parameter %r" % k)
        if k == "gravity":
            v = (C.c_double * 3)(*[float(x) for x in v])
        setattr(p, k, v)
    return p


def membrane_params(**params):
    """smg_membrane_params with the library's defaults and the given fields"""
    p = _lib.MembraneParamsC()
    _lib.load().smg_membrane_params_default(C.byref(p))
    for k, v in params.items():
        if k not in dict(p._fields_):
            raise TypeError("unknown membrane parameter %r" % k)
        setattr(p, k, v)
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the reference's free functions

def mg_precompute(V, F, ratio=0.25, nVCoarsest=500, dec_type=1, absorption_cap=0.0, keep_log=False):
    """mg_precompute(V, F, ratio, nVCoarsest, dec_type, mg)  (src/mg_precompute.cpp:15-87) -> Hierarchy.
    absorption_cap > 0: opt-in departure from the reference's collapse order (include/smg.h: smg_mg_precompute_capped).
    keep_log: keep the record of every collapse (the reference's decInfo), which query_coarse_to_fine needs."""
    L = _lib.load()
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    out = C.c_void_p()
    _chk(L.smg_mg_precompute_logged(_dp(V), V.shape[0], _ip(F), F.shape[0], ratio, nVCoarsest, dec_type, absorption_cap, int(bool(keep_log)),
                                    C.byref(out)), "smg_mg_precompute")
    return Hierarchy(handle=out.value)


def query_fine_to_coarse(mg, lv, face, bary):
    """query_fine_to_coarse (src/query_fine_to_coarse.cpp): points (face of level lv - 1's mesh, barycentric coordinates) -> (face of level
    lv's mesh, barycentric coordinates); the inverse of query_coarse_to_fine (needs keep_log=True)."""
    face = np.ascontiguousarray(face, dtype=np.int32)
    bary = np.ascontiguousarray(bary, dtype=np.float64).reshape(-1, 3)
    assert bary.shape[0] == face.shape[0]
    of = np.zeros(face.shape[0], dtype=np.int32)
    ob = np.zeros_like(bary)
    _chk(mg.L.smg_query_fine_to_coarse(mg.h, int(lv), face.shape[0], _ip(face), _dp(bary), _ip(of), _dp(ob)), "smg_query_fine_to_coarse")
    return of, ob


def query_coarse_to_fine(mg, lv, face, bary):
    """query_coarse_to_fine (src/query_coarse_to_fine.cpp): points (face of level lv's mesh, barycentric coordinates) -> (face of level
    lv - 1's mesh, barycentric coordinates) through the bijection of the decimation that built level lv (needs keep_log=True)."""
    face = np.ascontiguousarray(face, dtype=np.int32)
    bary = np.ascontiguousarray(bary, dtype=np.float64).reshape(-1, 3)
    assert bary.shape[0] == face.shape[0]
    of = np.zeros(face.shape[0], dtype=np.int32)
    ob = np.zeros_like(bary)
    _chk(mg.L.smg_query_coarse_to_fine(mg.h, int(lv), face.shape[0], _ip(face), _dp(bary), _ip(of), _dp(ob)), "smg_query_coarse_to_fine")
    return of, ob


def mg_precompute_block(V, F, ratio=0.25, nVCoarsest=500, dec_type=1):
    """mg_precompute_block (src/mg_precompute_block.cpp:23-95): P (x) I_3, DOF index 3*vertex + d."""
    L = _lib.load()
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    out = C.c_void_p()
    _chk(L.smg_mg_precompute_block(_dp(V), V.shape[0], _ip(F), F.shape[0], ratio, nVCoarsest, dec_type, C.byref(out)),
         "smg_mg_precompute_block")
    return Hierarchy(handle=out.value)


def mg_precompute_subdiv(V, F, n_sub, ratio=0.25, nVCoarsest=500, n_extra_levels=-1):
    """Hierarchy of a mid-point-subdivided mesh (benchmark configs C3/C5).  Returns (mg, V_fine, F_fine)."""
    L = _lib.load()
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    nV, nF = V.shape[0], F.shape[0]
    # closed-form sizes: every step adds one vertex per edge and quadruples the faces
    nv, nf = nV, nF
    he = set()
    if n_sub > 0:
        E0 = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
        ne = np.unique(E0, axis=0).shape[0]
        for _ in range(n_sub):
            nv, ne, nf = nv + ne, 2 * ne + 3 * nf, 4 * nf
    Vo = np.zeros((nv, 3))
    Fo = np.zeros((nf, 3), dtype=np.int32)
    out = C.c_void_p()
    _chk(L.smg_mg_precompute_subdiv(_dp(V), nV, _ip(F), nF, n_sub, ratio, nVCoarsest, n_extra_levels, C.byref(out),
                                    _dp(Vo), _ip(Fo)), "smg_mg_precompute_subdiv")
    return Hierarchy(handle=out.value), Vo, Fo


class min_quad_with_fixed_mg_data:
    """min_quad_with_fixed_mg_data (src/min_quad_with_fixed_mg.h:22-29); LHS/Auk live in the Hierarchy."""

    def __init__(self, mg):
        self.n = mg.n
        self.known = mg.known if mg.known is not None else np.zeros(0, np.int32)
        self.unknown = mg.unknown()


def min_quad_with_fixed_mg_precompute(A, known, mg):
    """min_quad_with_fixed_mg_precompute(A, [known,] data, mg, solver)  (src/min_quad_with_fixed_mg.cpp:3-51, :137-257).
    Returns `data`; the coarse `solver` is owned by `mg`."""
    mg.precompute(A, known)
    return min_quad_with_fixed_mg_data(mg)


def min_quad_with_fixed_mg_solve(data, RHS, known_val, z0, mg, tol=1e-3, maxIter=20, opts=None):
    """bool min_quad_with_fixed_mg_solve(data, RHS, [known_val,] z0, solver, [tol, [maxIter,]] mg, z, r_his)
    (src/min_quad_with_fixed_mg.cpp:80-135, :288-361).  Returns (converged, z, r_his)."""
    o = opts or SolveOpts(tol=tol, max_iter=maxIter)
    return mg.solve(RHS, z0, known_val, o)


def mg_VCycle(mg, B, preRelaxIter, postRelaxIter, lv, u):
    """mg_VCycle(solver, B, pre, post, lv, u, mg)  (src/mg_VCycle.cpp:3-59).  Returns the updated u."""
    return mg.vcycle(B, u, lv, preRelaxIter, postRelaxIter)
