"""Shared by tests/test_dgn_eig_cpu.py and tests/test_dgn_eig_gpu.py: the fp64 restatement of the Laplacians of
directional_gsn/data/HIV.py:21-51, the test graphs, and the bars a native eigenpair has to meet.

Eigenvectors are defined up to sign and up to rotation inside an eigenspace, so nothing here compares vectors element-wise: the bars
are eigenvalue error, residual, norm, orthogonality and the distance from the fp64 eigenspace of the eigenvalue's cluster."""
import numpy as np

EPS = 2.0 ** -24
NORMS = ("none", "sym", "walk")


def adjacency(n, ei):
    """A[u, v] = number of arcs u -> v of the graph-local edge_index (duplicates add, self loops count), float64."""
    A = np.zeros((n, n), dtype=np.float64)
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    np.add.at(A, (ei[0], ei[1]), 1.0)
    return A


def laplacian(n, ei, norm):
    """L of HIV.py:27-36 in float64, in the reference's own operation order (d = in-degree clipped at 1)."""
    A = adjacency(n, ei)
    d = A.sum(axis=0).astype(np.int64).clip(1)
    if norm == "none":
        return np.diag(d.astype(np.float64)) - A
    if norm == "sym":
        s = d ** -0.5
        return np.eye(n) - (s[:, None] * A) * s[None, :]
    if norm == "walk":
        return np.eye(n) - (d ** -1.0)[:, None] * A
    raise ValueError(norm)


def truth(n, ei, norm):
    """(all n eigenvalues ascending, their eigenvectors as columns) in float64.  'walk': the L_sym decomposition mapped by D^-1/2 and
    renormalised (L_walk = D^-1/2 L_sym D^1/2)."""
    if n == 0:
        return np.zeros(0), np.zeros((0, 0))
    if norm != "walk":
        return np.linalg.eigh(laplacian(n, ei, norm))
    lam, U = np.linalg.eigh(laplacian(n, ei, "sym"))
    d = adjacency(n, ei).sum(axis=0).clip(1)
    W = U / np.sqrt(d)[:, None]
    return lam, W / np.linalg.norm(W, axis=0, keepdims=True)


def clusters(lam, F):
    """Runs of eigenvalues whose neighbours differ by < 64 eps F: [(first, last + 1)]."""
    out, lo = [], 0
    for i in range(1, len(lam) + 1):
        if i == len(lam) or lam[i] - lam[i - 1] >= 64 * EPS * F:
            out.append((lo, i))
            lo = i
    return out


def cluster_of(lam, F, j):
    """(first, last + 1, gap to the rest of the spectrum) of the cluster that holds position j."""
    for lo, hi in clusters(lam, F):
        if lo <= j < hi:
            gap = np.inf
            if lo > 0:
                gap = min(gap, lam[lo] - lam[lo - 1])
            if hi < len(lam):
                gap = min(gap, lam[hi] - lam[hi - 1])
            return lo, hi, gap
    raise IndexError(j)


def off_space(v, B):
    """|v - P v|_2 for the orthogonal projector P onto the column span of B."""
    if B.shape[1] == 0:
        return float(np.linalg.norm(v))
    Q, _ = np.linalg.qr(B)
    return float(np.linalg.norm(v - Q @ (Q.T @ v)))


def dk_tolerance(F, gap):
    """Davis-Kahan applied to the residual bar: 2 * 32 eps F / gap."""
    return 2 * 32 * EPS * F / gap


def check_graph(n, ei, norm, vec, val, k, worst=None, what=""):
    """Every bar of one graph: vec [n, k], val [k] as the library returned them."""
    vec = np.asarray(vec, dtype=np.float64)
    val = np.asarray(val, dtype=np.float64)
    L = laplacian(n, ei, norm)
    F = float(np.linalg.norm(L))
    lam, U = truth(n, ei, norm)
    kk = min(k, n)
    assert np.all(vec[:, kk:] == 0) and np.all(np.isnan(val[kk:])), "%s: columns beyond n must be zero vectors with NaN values" % what
    w = worst if worst is not None else {}
    for j in range(kk):
        v = vec[:, j]
        e_val = abs(val[j] - lam[j]) / (EPS * F)
        e_res = np.linalg.norm(L @ v - val[j] * v) / (EPS * F)
        e_norm = abs(np.linalg.norm(v) - 1.0) / EPS
        lo, hi, gap = cluster_of(lam, F, j)
        tol = dk_tolerance(F, gap)
        assert tol <= 0.05, "%s: the test's own subspace tolerance is too loose (%g) for column %d" % (what, tol, j)
        e_sub = off_space(v, U[:, lo:hi])          # (1e-12 below: the rounding of this fp64 projection itself, for tol = 0)
        for key, x in (("val", e_val), ("res", e_res), ("norm", e_norm), ("sub/tol", e_sub / tol if tol > 0 else 0.0)):
            w[key] = max(w.get(key, 0.0), float(x))
        assert e_val <= 32, "%s: eigenvalue %d off by %.1f eps F" % (what, j, e_val)
        assert e_res <= 32, "%s: residual of pair %d is %.1f eps F" % (what, j, e_res)
        assert e_norm <= 64, "%s: norm of vector %d off by %.1f eps" % (what, j, e_norm)
        assert e_sub <= tol + 1e-12, "%s: vector %d is %g from its eigenspace (allowed %g)" % (what, j, e_sub, tol)
        i = int(np.argmax(np.abs(v)))         # (argmax: the first of equal magnitudes)
        assert v[i] > 0, "%s: sign convention, vector %d" % (what, j)
    if norm != "walk" and kk:
        e_orth = np.abs(vec[:, :kk].T @ vec[:, :kk] - np.eye(kk)).max() / EPS
        w["orth"] = max(w.get("orth", 0.0), float(e_orth))
        assert e_orth <= 1024, "%s: |V^T V - I| = %.0f eps" % (what, e_orth)
    return w


# ----------------------------------------------------------------------------------------------------------------
# graphs: (n, graph-local edge_index [2, E] with both directions of every edge)
# ----------------------------------------------------------------------------------------------------------------
def both(n, und):
    und = np.asarray(und, dtype=np.int64).reshape(-1, 2)
    return n, np.ascontiguousarray(np.concatenate([und, und[:, ::-1]], axis=0).T)


def path(n, off=0):
    return [(off + i, off + i + 1) for i in range(n - 1)]


def cycle(n, off=0):
    return path(n, off) + [(off + n - 1, off)]


def known_graphs():
    """Graphs of at most 9 vertices with known, mostly degenerate, spectra."""
    g = {
        "P6": both(6, path(6)), "P9": both(9, path(9)), "C6": both(6, cycle(6)), "C7": both(7, cycle(7)),
        "star7": both(7, [(0, i) for i in range(1, 7)]),
        "K6": both(6, [(i, j) for i in range(6) for j in range(i + 1, 6)]),
        "two_components": both(9, cycle(5) + path(4, 5)),
        "P5_isolated": both(6, path(5)),
        "C6_doubled_edge": both(6, cycle(6) + [(0, 1)]),
    }
    return g


def tree_with_rings(n, seed, rings=3):
    """A random recursive tree on n vertices plus a few ring closures."""
    rng = np.random.default_rng(seed)
    und = {(int(rng.integers(v)), v) for v in range(1, n)}
    for _ in range(rings if n > 4 else 0):
        a, b = (int(x) for x in rng.integers(n, size=2))
        if a != b:
            und.add((min(a, b), max(a, b)))
    return both(n, sorted(und))


BOUNDARY_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160)
# the seed of each size: chosen on fp64 alone so that the subspace tolerance of every tested cluster is <= 0.05 for the three norms
BOUNDARY_SEEDS = {160: 1}


def boundary_graphs():
    return {n: tree_with_rings(n, BOUNDARY_SEEDS.get(n, 0)) for n in BOUNDARY_SIZES}
