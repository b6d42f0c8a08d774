"""Shared workload builders for the tests: the reference demos' systems on small meshes.
Caller-side numerics come from the numpy restatement (oracle/mesh_np.py) so that the oracle and the HIP path
see bit-identical inputs."""
import numpy as np
import scipy.sparse as sp

from oracle import mesh_np as M


def subdiv_problem(mesh="ogre_sim.smgm", n_sub=2, kind="mcf", k=1, seed=0, n_pins=0):
    """Returns dict(A, Ps, RHS, z0, known, known_val, V, F).
    kind 'mcf'    : LHS = M_bary - 0.01 L, RHS = M * X (05_example_mean_curvature_flow/main.cpp:66-69), no constraints
    kind 'poisson': A = -L, B = M_voronoi * 1 (03_mg_solver/main.cpp:44-61), constraints = boundary loop
                    (or n_pins random vertices on a closed mesh, 04_mg_solver_nobd/main.cpp:73-94)."""
    rng = np.random.default_rng(seed)
    if mesh == "torus":
        V, F = M.torus(24, 16)
    else:
        V, F = M.read_smgm(mesh)
    V = M.normalize_unit_area(V, F)
    Vf, Ff, Ps = M.subdivision_hierarchy(V, F, n_sub)
    n = Vf.shape[0]
    L = M.cotmatrix(Vf, Ff)
    out = dict(V=Vf, F=Ff, Ps=Ps)
    if kind == "mcf":
        Mb = M.massmatrix(Vf, Ff, "barycentric")
        A = (Mb - 0.01 * L).tocsr()
        X = Vf if k == 3 else np.concatenate([Vf, rng.uniform(-1, 1, (n, max(k - 3, 0)))], axis=1)[:, :k]
        out.update(A=A, RHS=np.asfortranarray(Mb @ X), z0=np.asfortranarray(X.copy()), known=None, known_val=None)
    else:
        A = (-L).tocsr()
        Mv = M.massmatrix(Vf, Ff, "voronoi")
        b = M.boundary_loop(Ff)
        if n_pins > 0 or len(b) == 0:
            b = rng.choice(n, size=max(n_pins, 8), replace=False).astype(np.int32)
        B = np.repeat((Mv @ np.ones(n))[:, None], k, axis=1)
        if k > 1:
            B = B * rng.uniform(0.5, 1.5, (1, k))
        bval = np.zeros((len(b), k))
        B[b, :] = bval
        z0 = rng.uniform(-1, 1, (n, k))
        out.update(A=A, RHS=np.asfortranarray(B), z0=np.asfortranarray(z0), known=b, known_val=bval)
    A.sort_indices()
    return out


def value_step(A, seed):
    """What a time-stepping caller hands to its next smg_precompute: the pattern of A, new values, still SPD, and NOT bit-symmetric.
    D A D + diag(u diag A) with D = 1 + 0.01 U(0,1) and u ~ U(0, 0.5) -- which differs from its transpose in the last bits only -- and then every
    stored entry moved independently of its mirror image by 1 + 1e-5 U(-1,1), so that a sweep on A where A^T is due (the reference walks
    column i) gives other bits in every row."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    D = sp.diags(1.0 + 0.01 * rng.uniform(size=n))
    B = (D @ A @ D + sp.diags(rng.uniform(0, 0.5, n) * A.diagonal())).tocsr()
    B.sort_indices()
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    B.data = B.data * (1.0 + 1e-5 * rng.uniform(-1, 1, B.nnz))
    return B


def random_spd_hierarchy(rng, n, levels, hub):
    """A random sparse SPD matrix (irregular degrees; optionally a few hub rows so that SELL slices get very wide and the
    compact-panel fallback and > 4 colours are exercised) with a random aggregation-type prolongation hierarchy."""
    deg = rng.integers(2, 9, n)
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, rows.size)
    if hub:
        hubs = rng.choice(n, 3, replace=False)
        extra = rng.choice(n, (3, min(n - 1, 120)))
        rows = np.concatenate([rows, np.repeat(hubs, extra.shape[1])]); cols = np.concatenate([cols, extra.ravel()])
    W = sp.coo_matrix((-rng.uniform(0.1, 1.0, rows.size), (rows, cols)), shape=(n, n)).tocsr()
    W.setdiag(0); W.eliminate_zeros()
    W = W + W.T
    A = (W + sp.diags(np.asarray(-W.sum(axis=1)).ravel() + rng.uniform(0.05, 0.5, n))).tocsr()   # strictly diagonally dominant
    A.sort_indices()
    Ps, m = [], n
    for _ in range(levels - 1):
        mc = max(2, m // 3)
        agg = rng.integers(0, mc, m); agg[:mc] = np.arange(mc)          # every coarse vertex has a child
        second = rng.integers(0, mc, m)
        w = rng.uniform(0.5, 1.0, m)
        P = sp.coo_matrix((np.concatenate([w, 1 - w]), (np.concatenate([np.arange(m)] * 2), np.concatenate([agg, second]))), shape=(m, mc)).tocsr()
        P.sum_duplicates(); P.sort_indices()
        Ps.append(P); m = mc
    return A, Ps


def random_block_system(W, rng, keep=1.0, diag_only_frac=0.0):
    """A 3-DOF SPD system on the vertex graph of W (a scalar symmetric matrix: its off-diagonal pattern is the graph), DOF index 3 v + d,
    with 3 x 3 blocks that are NOT all full -- what the mesh systems and kron(S, B) never give the block kernels:
      off-diagonal blocks  B_ij = |W_ij| U(-1,1)^{3x3} for i < j and B_ji = B_ij^T; every entry is stored with probability `keep` (the mirror
                           block gets the transposed mask: the scalar pattern stays symmetric), one entry per block always, so that every
                           edge of the graph keeps its block;
      diagonal blocks      a symmetric coupling U(-0.3, 0.3) on (0,1), (0,2), (1,2) -- stored on none of them on a fraction `diag_only_frac`
                           of the vertices, whose diagonal block then holds its three diagonal entries and nothing else;
      diagonal entries     the scalar row's absolute off-diagonal sum plus U(0.05, 0.5): strictly diagonally dominant and symmetric => SPD.
    Entries that are masked out are not stored at all (no explicit zeros).  Returns the 3n x 3n CSR matrix, indices sorted."""
    W = sp.coo_matrix(W)
    n = W.shape[0]
    up = W.row < W.col
    ei, ej, ew = W.row[up], W.col[up], np.abs(W.data[up])
    m = len(ei)
    B = ew[:, None, None] * rng.uniform(-1, 1, (m, 3, 3))
    mask = rng.uniform(size=(m, 3, 3)) < keep
    forced = rng.integers(0, 9, m)
    mask[np.arange(m), forced // 3, forced % 3] = True
    q, d, e = np.nonzero(mask)
    rows = [3 * ei[q] + d, 3 * ej[q] + e]
    cols = [3 * ej[q] + e, 3 * ei[q] + d]
    vals = [B[q, d, e], B[q, d, e]]
    coupled = np.flatnonzero(rng.uniform(size=n) >= diag_only_frac)
    for d, e in ((0, 1), (0, 2), (1, 2)):
        c = rng.uniform(-0.3, 0.3, len(coupled))
        rows += [3 * coupled + d, 3 * coupled + e]; cols += [3 * coupled + e, 3 * coupled + d]; vals += [c, c]
    off = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * n, 3 * n))
    diag = np.asarray(abs(off).sum(axis=1)).ravel() + rng.uniform(0.05, 0.5, 3 * n)
    A = (off + sp.diags(diag)).tocsr()
    A.sort_indices()
    assert A.nnz == off.nnz + 3 * n and (A != A.T).nnz == 0
    return A


def kron3_prolongs(Ps):
    """P (x) I_3 of every prolongation of a vertex hierarchy (row 3 r + d holds P(r, c) at column 3 c + d), indices sorted"""
    out = []
    for P in Ps:
        K = sp.kron(sp.csr_matrix(P), sp.identity(3), format="csr")
        K.sort_indices()
        out.append(K)
    return out


# The block systems off the mesh (tests/test_gpu_block_shapes.py, the block-* builders of tests/test_gpu_f32_cycle.py): name ->
# (seed, vertices, levels, hub rows, keep, diag_only_frac) on random_spd_hierarchy graphs; "path-<n>" / "path-<n>-3lv": the path graph.
BLOCK_SHAPES = {
    "random": (1, 200, 2, False, 1.0, 0.0),
    "random-sparse-blocks": (2, 777, 3, False, 0.6, 0.3),
    "hub": (3, 1500, 3, True, 0.6, 0.3),
    "under-half-fill": (5, 65, 2, False, 0.35, 0.5),
    "hub-wide-k": (7, 300, 3, True, 1.0, 0.0),
}
_BLOCK_SYSTEMS = {}


def block_shape_system(name):
    """(A, [P (x) I_3 ...]) of a named block system; built once per process, to be left unchanged"""
    if name not in _BLOCK_SYSTEMS:
        if name.startswith("path-"):
            part = name.split("-")
            n, levels = int(part[1]), 3 if part[-1] == "3lv" else 2
            Ps, m = [], n
            for _ in range(levels - 1):
                Ps.append(_path_interp(m)); m = (m + 1) // 2
            A = random_block_system(_path_matrix(n), np.random.default_rng(100 + n), 0.7, 0.3)
        else:
            seed, n, levels, hub, keep, diag_only = BLOCK_SHAPES[name]
            rng = np.random.default_rng(seed)
            W, Ps = random_spd_hierarchy(rng, n, levels, hub)
            A = random_block_system(W, rng, keep, diag_only)
        _BLOCK_SYSTEMS[name] = (A, kron3_prolongs(Ps))
    return _BLOCK_SYSTEMS[name]


def _path_matrix(n):
    """the tiny and ragged systems: a path graph's diagonally dominant matrix"""
    return sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n)).tocsr()


def _path_interp(n):
    """linear interpolation from every second vertex of the path"""
    nc = (n + 1) // 2
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 2 == 0:
            rows.append(i); cols.append(i // 2); vals.append(1.0)
        else:
            rows += [i, i]; cols += [i // 2, min(i // 2 + 1, nc - 1)]; vals += [0.5, 0.5]
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, nc))
