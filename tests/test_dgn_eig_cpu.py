"""Laplacian eigenvector fields of the directional GSN, the parts that need no GPU: the fp64 Laplacians the GPU tests measure against
are the reference's own (tests/golden/dgn_eig.npz records the matrices data/HIV.py:27-36 handed to ARPACK), the argument errors come
before the library is needed, and the library exports the solver."""
import os

import numpy as np
import pytest

import dgn_eig_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "dgn_eig.npz"))


def test_fp64_laplacians_equal_the_reference_s_exactly(golden):
    """Pins the clip of the degree, the three norms and the orientation to the reference's own lines: every recorded L, bit for bit."""
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 36 and {n.split("/")[1] for n in names} == set(R.NORMS)
    for name in names:
        n, ei = int(golden[name + "/n"]), golden[name + "/edge_index"]
        L = R.laplacian(n, ei, name.split("/")[1])
        assert L.dtype == np.float64 and np.array_equal(L, golden[name + "/L"]), name
    # the cases that make the definition bite are in the fixture: an isolated vertex (clip: its diagonal entry is 1) and a doubled arc pair
    assert golden["P5_isolated/none/L"][5, 5] == 1.0 and golden["C6_doubled_edge/none/L"][0, 1] == -2.0


def test_test_graphs_keep_the_subspace_tolerance_tight():
    """The Davis-Kahan tolerance of every cluster the GPU tests check is <= 0.05 on fp64 (a loose bound could hide a failure)."""
    graphs = list(R.known_graphs().values()) + list(R.boundary_graphs().values())
    for n, ei in graphs:
        for norm in R.NORMS:
            lam, _ = R.truth(n, ei, norm)
            F = float(np.linalg.norm(R.laplacian(n, ei, norm)))
            for j in range(min(4, n)):
                assert R.dk_tolerance(F, R.cluster_of(lam, F, j)[2]) <= 0.05, (n, norm, j)


def test_walk_truth_is_the_eigen_decomposition_of_l_walk():
    n, ei = R.tree_with_rings(17, 0)
    lam, W = R.truth(n, ei, "walk")
    L = R.laplacian(n, ei, "walk")
    assert np.abs(L @ W - W * lam[None, :]).max() < 1e-13 and np.allclose(np.linalg.norm(W, axis=0), 1.0)


def test_argument_errors_come_before_the_library():
    from gsn_amd import dgn, synth
    b = synth.zinc_shape_batch(3, seed=1)
    for kw in (dict(norm="rw"), dict(norm=None), dict(k=0), dict(k=9), dict(k=2.5), dict(max_sweeps=0), dict(max_sweeps=65),
               dict(max_sweeps=None)):
        with pytest.raises(ValueError):
            dgn.laplacian_eigenvectors(b, **kw)
    with pytest.raises(NotImplementedError, match="direction laplacian is not currently supported."):
        dgn.DGNGraph.from_batch(b, directions=["eig", "laplacian"])
    with pytest.raises(ValueError):
        dgn.DGNGraph.from_batch(b, directions=["eig"], norm="rw")
    with pytest.raises(ValueError):
        dgn.DGNGraph.from_batch(b, directions=["subgraphs"])
    with pytest.raises(ValueError):
        dgn.DGNGraph.from_batch(b, directions=["edge_feat"])
    bad = synth.Batch(b.node_ptr[::-1].copy(), b.edge_ptr, b.edge_index)
    with pytest.raises(ValueError):
        dgn.laplacian_eigenvectors(bad)


def test_solver_is_exported_and_typed():
    import ctypes
    from gsn_amd import _abi
    _abi.build()
    raw = ctypes.CDLL(os.path.join(REPO, "gsn_amd", "lib", "libgsn_hip.so"))
    for name in ("gsn_laplacian_eig_hip", "gsn_laplacian_eig_scratch_floats"):
        assert hasattr(raw, name) and name in _abi.SIGNATURES
    assert len(_abi.SIGNATURES["gsn_laplacian_eig_hip"][1]) == 18
    lib = _abi.lib()
    assert lib.gsn_laplacian_eig_scratch_floats(256, 3) == 3 * 2 * 256 * 257
    assert [lib.gsn_laplacian_eig_scratch_floats(c, 3) for c in (32, 64, 128)] == [0, 0, 0]
    # argument errors of the entry point itself: no launch, a message
    assert lib.gsn_laplacian_eig_hip(1, None, None, None, 0, None, 0, 48, 0, 4, 16, None, None, None, None, None, 0, None) == -1
    assert b"n_class" in lib.gsn_last_error()
    assert lib.gsn_laplacian_eig_hip(1, None, None, None, 0, None, 0, 32, 0, 9, 16, None, None, None, None, None, 0, None) == -1
    assert lib.gsn_laplacian_eig_hip(1, None, None, None, 0, None, 0, 32, 0, 4, 0, None, None, None, None, None, 0, None) == -1
    assert lib.gsn_laplacian_eig_hip(1, None, None, None, 0, None, 0, 32, 3, 4, 16, None, None, None, None, None, 0, None) == -1
