"""A numpy restatement of the pieces of the V-cycle as the SELL kernels compute them (csrc/smg_device.hip: k_sell, k_sell_wide, k_long_ax;
csrc/smg_bsr3_device.hip), generic over the arithmetic: dtype = np.float64 is the reference's (and the oracle's), dtype = np.float32 the
mixed-precision cycle's.  TEST INFRASTRUCTURE ONLY.

What the kernels promise, and what is restated here:
  * a row's sum starts from +0 and takes its stored entries in ascending column order, one rounded multiplication and one rounded addition
    per entry (the library is built with -ffp-contract=off): acc = acc + a_ij * x_j;
  * the smoothers leave the diagonal entry out of the sum and divide by it:
        Gauss-Seidel  u_i = (b_i - s_i) / a_ii          (rows in ascending order, a colour at a time: rows of a colour do not couple)
        Jacobi        t = (b_i - s_i) / a_ii,  u_i = u_i + omega * (t - u_i)
        Chebyshev     r = t - u_i,  d_i = c1 * d_i + c2 * r  (step 0: d_i = c2 * r),  u_i = u_i + d_i
    with omega, c1, c2 computed in fp64 (cheby_coefs of csrc/smg_cycle.cpp) and rounded to dtype once, as the launch arguments are;
  * the smoothers stream A^T (the reference walks column i of A, src/mg_VCycle.cpp:149-155): pass G = A.T where A is not symmetric bit for bit;
  * the fp32 images are the fp64 values rounded to nearest: np.float32(value).
The array operations below act on arrays of dtype, so numpy rounds every single operation to dtype.

Matrices are scipy CSR with sorted indices; vectors are (n, k) arrays."""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24                   # unit roundoff of fp32


def gamma32(N):
    """gamma_N = N u / (1 - N u) for fp32: the relative bound of a sum of N rounded products in any order (Higham, Accuracy and Stability, 3.1)"""
    N = np.asarray(N, dtype=np.float64)
    return N * U32 / (1.0 - N * U32)


class Ell:
    """The rows `rows` (default: all) of a CSR matrix as padded columns: slot j of every row that has one, ascending column order.
    Rows are kept sorted by decreasing length so that slot j is a prefix operation."""

    def __init__(self, M, dtype, rows=None):
        M = sp.csr_matrix(M)
        if not M.has_sorted_indices:
            M = M.sorted_indices()
        self.dtype = np.dtype(dtype)
        self.shape = M.shape
        rows = np.arange(M.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
        lens = (M.indptr[rows + 1] - M.indptr[rows]).astype(np.int64)
        order = np.argsort(-lens, kind="stable")
        self.rows, lens = rows[order], lens[order]
        self.lens = lens
        w = int(lens.max()) if len(lens) else 0
        self.w = w
        m = len(rows)
        self.col = np.zeros((m, w), dtype=np.int64)
        self.val = np.zeros((m, w), dtype=self.dtype)
        mask = np.arange(w)[None, :] < lens[:, None]
        idx = (M.indptr[self.rows].astype(np.int64)[:, None] + np.arange(w)[None, :])[mask]
        self.col[mask] = M.indices[idx]
        self.val[mask] = M.data[idx].astype(self.dtype)          # round to nearest: the device's cast
        self.count = [int(np.count_nonzero(lens > j)) for j in range(w)]   # rows that have a slot j: a prefix
        isd = mask & (self.col == self.rows[:, None])
        self.has_diag = isd.any(axis=1)
        self.diag = np.ones(m, dtype=self.dtype)                 # (a row without a stored diagonal divides by 1, as the kernels do)
        self.diag[self.has_diag] = self.val[isd]

    def sums(self, x, skip_diag=False):
        """s_i = sum_j a_ij x_j over the stored entries in ascending column order (skip_diag: without the diagonal entry), rows in self.rows order"""
        x = np.asarray(x)
        assert x.dtype == self.dtype and x.ndim == 2
        acc = np.zeros((len(self.rows), x.shape[1]), dtype=self.dtype)
        for j in range(self.w):
            m = self.count[j]
            c = self.col[:m, j]
            p = self.val[:m, j][:, None] * x[c]                  # one rounded product ...
            s = acc[:m] + p                                       # ... one rounded addition
            if skip_diag:
                s = np.where((c == self.rows[:m])[:, None], acc[:m], s)
            acc[:m] = s
        return acc

    def abs_sums(self, x):
        """sum_j |a_ij| |x_j| in fp64 on the operands as they are stored (rounded to dtype), rows in natural order"""
        out = np.zeros((len(self.rows), x.shape[1]))
        ax = np.abs(np.asarray(x, dtype=np.float64))
        for j in range(self.w):
            m = self.count[j]
            out[:m] += np.abs(self.val[:m, j].astype(np.float64))[:, None] * ax[self.col[:m, j]]
        return self._natural(out)

    def sums64(self, x):
        """the same sums in fp64 on the operands as they are stored, rows in natural order"""
        out = np.zeros((len(self.rows), x.shape[1]))
        x64 = np.asarray(x, dtype=np.float64)
        for j in range(self.w):
            m = self.count[j]
            out[:m] += self.val[:m, j].astype(np.float64)[:, None] * x64[self.col[:m, j]]
        return self._natural(out)

    def row_lengths(self):
        out = np.zeros(self.shape[0], dtype=np.int64)
        out[self.rows] = self.lens
        return out

    def _natural(self, a):
        out = np.zeros((self.shape[0],) + a.shape[1:], dtype=a.dtype)
        out[self.rows] = a
        return out


def _as(x, dtype):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    assert x.dtype == np.dtype(dtype), "operands must already be of the arithmetic's dtype (round them where the cycle rounds them)"
    return x


def spmv(E, x):
    """y = A x"""
    return E._natural(E.sums(_as(x, E.dtype)))


def resid(E, b, x):
    """r = b - A x"""
    return _as(b, E.dtype) - spmv(E, x)


def restrict(E_PT, r):
    """bc = PT r"""
    return spmv(E_PT, r)


def prolong_add(E_P, u, uc):
    """u + P uc"""
    return _as(u, E_P.dtype) + spmv(E_P, uc)


class GsSchedule:
    """The order of a forward Gauss-Seidel sweep as batches of rows that can be updated together: rows in ascending order, colour_ptr = the
    row offsets of blocks swept one after the other (None: the whole matrix is one block, the lexicographic sweep).  Inside a block row i
    reads the NEW value of every coupled row j < i and the OLD value of every coupled row j > i; the batches are the level sets of that
    dependency (a colour of a scalar colouring is one batch, a vertex colour of a 3-DOF block hierarchy three)."""

    def __init__(self, G, dtype, colour_ptr=None):
        G = sp.csr_matrix(G)
        if not G.has_sorted_indices:
            G = G.sorted_indices()
        n = G.shape[0]
        cp = np.array([0, n]) if colour_ptr is None else np.asarray(colour_ptr, dtype=np.int64)
        assert cp[0] == 0 and cp[-1] == n
        coo = G.tocoo()
        r, c = coo.row.astype(np.int64), coo.col.astype(np.int64)
        block = np.searchsorted(cp, np.arange(n), side="right") - 1
        intra = (block[r] == block[c]) & (r != c)
        lo_r, lo_c = r[intra & (c < r)], c[intra & (c < r)]      # r reads the new value of c: after it
        hi_r, hi_c = r[intra & (c > r)], c[intra & (c > r)]      # r reads the old value of c: c not before r
        level = np.zeros(n, dtype=np.int64)
        while True:
            new = level.copy()
            if len(lo_r):
                np.maximum.at(new, lo_r, level[lo_c] + 1)
            if len(hi_r):
                np.maximum.at(new, hi_c, level[hi_r])
            if np.array_equal(new, level):
                break
            level = new
        key = block * (int(level.max()) + 1 if n else 1) + level
        order = np.argsort(key, kind="stable")
        cuts = np.flatnonzero(np.diff(key[order])) + 1
        self.batches = [Ell(G, dtype, rows=rows) for rows in np.split(order, cuts)]
        self.dtype = np.dtype(dtype)


def gauss_seidel(S, b, u, iters):
    """`iters` forward sweeps of schedule S: u_i = (b_i - s_i) / a_ii"""
    b, u = _as(b, S.dtype), _as(u, S.dtype).copy()
    for _ in range(iters):
        for E in S.batches:
            u[E.rows] = (b[E.rows] - E.sums(u, skip_diag=True)) / E.diag[:, None]
    return u


def jacobi(E, b, u, iters, omega):
    """`iters` damped-Jacobi sweeps, every row from the old iterate"""
    b, u = _as(b, E.dtype), _as(u, E.dtype).copy()
    om = E.dtype.type(omega)
    for _ in range(iters):
        xi = u[E.rows]
        t = (b[E.rows] - E.sums(u, skip_diag=True)) / E.diag[:, None]
        new = np.empty_like(u)
        new[E.rows] = xi + om * (t - xi)
        u = new
    return u


def spectral_bound(G):
    """max_i (sum_j |g_ij|) / g_ii in fp64, the row sums in ascending column order: the Gershgorin bound of D^-1 A the Chebyshev smoother uses"""
    E = Ell(G, np.float64)
    acc = np.zeros(len(E.rows))
    for j in range(E.w):
        m = E.count[j]
        acc[:m] = acc[:m] + np.abs(E.val[:m, j])
    ok = E.has_diag & (E.diag > 0.0)
    return float(np.max(acc[ok] / E.diag[ok])) if ok.any() else 0.0


def cheby_coefs(lam, frac, degree):
    """(c1, c2) of step s = 0 .. degree - 1 in fp64: the statements of cheby_coefs (csrc/smg_cycle.cpp) in their order"""
    lmax, lmin = lam, lam * frac
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    out = []
    for s in range(degree):
        if s == 0:
            out.append((0.0, 1.0 / theta))
        else:
            rho_new = 1.0 / (2.0 * sigma - rho)
            out.append((rho_new * rho, 2.0 * rho_new / delta))
            rho = rho_new
    return out


def chebyshev(E, b, u, iters, lam, frac):
    """relax(iters) of a Chebyshev-Jacobi level: one polynomial of degree iters + 1 (nothing for iters <= 0)"""
    b, u = _as(b, E.dtype), _as(u, E.dtype).copy()
    if iters <= 0:
        return u
    T = E.dtype.type
    d = np.zeros_like(u)
    for c1, c2 in cheby_coefs(lam, frac, iters + 1):
        c1, c2 = T(c1), T(c2)                    # the launch arguments: fp64 coefficients rounded once
        xi = u[E.rows]
        t = (b[E.rows] - E.sums(u, skip_diag=True)) / E.diag[:, None]
        r = t - xi
        dn = c1 * d[E.rows] + c2 * r if c1 != T(0) else c2 * r
        new, dnew = np.empty_like(u), np.empty_like(u)
        new[E.rows] = xi + dn
        dnew[E.rows] = dn
        u, d = new, dnew
    return u


def product_sum_bound(E, x, exact_result=None):
    """gamma_32(w_i) * sum_j |a_ij| |x_j| per row: how far an fp32 sum of row i's w_i products, in any order, may lie from the exact sum of
    the stored operands (w_i rounded products, w_i - 1 rounded additions: the first addition is to +0).
    exact_result (b - A x, u + P uc): the op ends with one more rounded addition, fl(b -+ s) = (b -+ s)(1 + d), |d| <= u: with s = s_exact + e
    that is |fl - exact| <= |e| (1 + u) + u |exact|."""
    bound = gamma32(np.maximum(E.row_lengths(), 1))[:, None] * E.abs_sums(x)
    if exact_result is not None:
        bound = bound * (1.0 + U32) + U32 * np.abs(exact_result)
    return bound
