"""Laplacian eigenvector fields (gsn_amd.dgn.laplacian_eigenvectors, csrc/eig.hip) against float64.

Eigenvectors are defined up to sign and up to rotation inside an eigenspace, and the reference calls ARPACK with tol=1e-2 and a random
start: nothing here compares vectors element-wise.  tests/dgn_eig_ref.py states the bars (eps = 2^-24, F = |L|_F):
|lambda - lambda_ref| <= 32 eps F, |L v - lambda v| <= 32 eps F, | |v| - 1 | <= 64 eps, |V^T V - I| <= 1024 eps ('none', 'sym'), the
distance of v from the float64 eigenspace of its eigenvalue's cluster <= 2 * 32 eps F / gap (Davis-Kahan; asserted <= 0.05), the
sign convention, bit-identical repeats, sweeps_used <= max_sweeps and no status."""
import os

import numpy as np
import pytest
import torch

import dgn_eig_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4
MAX_SWEEPS = 16


def run(batch, norm, k=K, max_sweeps=MAX_SWEEPS):
    """(vec, val, status, sweeps) as numpy arrays, check=False."""
    from gsn_amd import dgn
    out = dgn.laplacian_eigenvectors(batch, k=k, norm=norm, max_sweeps=max_sweeps, check=False, return_values=True, return_sweeps=True)
    return tuple(t.cpu().numpy() for t in out)


def check_batch(graphs, norm, what, k=K):
    """One call over `graphs` [(n, ei)], every graph against float64; the call repeated must give the same bits."""
    from gsn_amd import synth
    b = synth.collate(graphs)
    vec, val, status, sweeps = run(b, norm, k)
    again = run(b, norm, k)
    assert vec.tobytes() == again[0].tobytes() and val.tobytes() == again[1].tobytes(), "%s: two runs differ" % what
    assert vec.dtype == np.float32 and vec.shape == (b.num_nodes, k) and val.shape == (b.num_graphs, k)
    assert not status.any(), "%s: status %s" % (what, status.tolist())
    assert sweeps.max(initial=0) <= MAX_SWEEPS
    worst = {"sweeps": int(sweeps.max(initial=0))}
    for g, (n, ei) in enumerate(graphs):
        R.check_graph(n, ei, norm, vec[b.node_ptr[g]:b.node_ptr[g + 1]], val[g], k, worst, "%s graph %d (n = %d, %s)" % (what, g, n, norm))
    print("worst over %s / %s: %s" % (what, norm, {key: round(x, 3) for key, x in worst.items()}))
    return vec, val, b


@pytest.mark.parametrize("norm", R.NORMS)
def test_known_spectra(norm):
    """Paths, cycles (double eigenvalues), a star and K6 (one eigenvalue n - 1 times), two components (two zero eigenvalues), an
    isolated vertex (the clip), a doubled edge: the degenerate clusters are where a rotation scheme goes wrong first."""
    graphs = R.known_graphs()
    vec, val, b = check_batch(list(graphs.values()), norm, "known spectra")
    names = list(graphs)
    if norm == "none":
        assert np.allclose(val[names.index("C6")], [0, 1, 1, 3], atol=1e-5) and np.allclose(val[names.index("K6")], [0, 6, 6, 6], atol=1e-5)
        assert np.allclose(val[names.index("two_components")][:2], 0, atol=1e-5)
        assert np.allclose(val[names.index("P9")], 2 - 2 * np.cos(np.pi * np.arange(4) / 9), atol=1e-5)


@pytest.mark.parametrize("norm", R.NORMS)
def test_class_boundaries_alone_and_batched(norm):
    """n = 1, 2, 3 (fewer vertices than columns), then both sides of every class boundary (32 / 64 / 128) and one graph of the scratch
    class: each alone, and all in one shuffled batch whose rows must equal the stand-alone rows bit for bit (order restoration, offsets,
    class grouping)."""
    graphs = R.boundary_graphs()
    alone = {}
    for n, gr in graphs.items():
        vec, val, _ = check_batch([gr], norm, "n = %d alone" % n)
        alone[n] = (vec, val)
    order = list(graphs)
    np.random.default_rng(5).shuffle(order)
    assert order != sorted(order)
    from gsn_amd import synth
    b = synth.collate([graphs[n] for n in order])
    vec, val, status, sweeps = run(b, norm)
    assert not status.any() and sweeps.max() <= MAX_SWEEPS
    for g, n in enumerate(order):
        assert vec[b.node_ptr[g]:b.node_ptr[g + 1]].tobytes() == alone[n][0].tobytes(), "rows of n = %d differ in the batch" % n
        assert val[g].tobytes() == alone[n][1][0].tobytes(), "values of n = %d differ in the batch" % n
    for n in (1, 2, 3):
        assert np.isnan(alone[n][1][0, n:]).all() and not np.isnan(alone[n][1][0, :n]).any() and (alone[n][0][:, n:] == 0).all()


@pytest.mark.parametrize("norm", R.NORMS)
def test_molecule_shaped_batch(norm):
    from gsn_amd import synth
    b = synth.zinc_shape_batch(300, seed=0)
    check_batch([b.graph(g) for g in range(b.num_graphs)], norm, "300 molecules")


def test_more_columns_than_four():
    """k = 8 (GSN_EIG_KMAX) and k = 1."""
    graphs = [R.tree_with_rings(12, 3), R.tree_with_rings(40, 0), R.tree_with_rings(70, 0)]
    for k in (1, 8):
        for n, ei in graphs:
            lam, _ = R.truth(n, ei, "none")
            F = float(np.linalg.norm(R.laplacian(n, ei, "none")))
            assert all(R.dk_tolerance(F, R.cluster_of(lam, F, j)[2]) <= 0.05 for j in range(k))
        check_batch(graphs, "none", "k = %d" % k, k=k)


def test_against_the_reference_s_own_output():
    """tests/golden/dgn_eig.npz: the matrices the reference handed to ARPACK and the [n, 4] tensors it got back.  The native eigenvalues
    meet the bar against the recorded L; every reference vector lies in the span of the native vectors of its cluster (the float64
    cluster space where the k-th position cuts the cluster or ARPACK returned an eigenvalue beyond the four smallest) up to its own
    measured deviation delta plus the Davis-Kahan tolerance."""
    from gsn_amd import synth
    z = np.load(os.path.join(REPO, "tests", "golden", "dgn_eig.npz"))
    names = [str(n) for n in z["names"]]
    for norm in R.NORMS:
        cases = [n for n in names if n.endswith("/" + norm)]
        graphs = [(int(z[c + "/n"]), z[c + "/edge_index"]) for c in cases]
        b = synth.collate(graphs)
        vec, val, status, _ = run(b, norm)
        assert not status.any()
        for g, c in enumerate(cases):
            n, ei = graphs[g]
            L = z[c + "/L"]
            F = float(np.linalg.norm(L))
            lam = np.linalg.eigvalsh(L) if norm != "walk" else np.sort(np.real(np.linalg.eigvals(L)))
            assert np.abs(val[g].astype(np.float64) - lam[:K]).max() <= 32 * R.EPS * F, c
            lam_t, U = R.truth(n, ei, norm)
            assert np.abs(lam_t - lam).max() < 1e-12
            mine = vec[b.node_ptr[g]:b.node_ptr[g + 1]].astype(np.float64)
            for j in range(K):
                pos = int(np.argmin(np.abs(lam - z[c + "/val"][j])))
                lo, hi, gap = R.cluster_of(lam, F, pos)
                tol = R.dk_tolerance(F, gap)
                assert tol <= 0.05, (c, j, tol)
                space = mine[:, lo:hi] if hi <= K else U[:, lo:hi]
                dev = R.off_space(z[c + "/eig"][:, j].astype(np.float64), space)
                assert dev <= float(z[c + "/delta"][j]) + tol + 1e-12, "%s: reference vector %d is %g from the native space (allowed %g + %g)" % (
                    c, j, dev, float(z[c + "/delta"][j]), tol)


def test_statuses():
    from gsn_amd import dgn, synth
    good = [R.tree_with_rings(n, 7) for n in (9, 14, 40, 70)]
    asym = (6, R.both(6, R.path(6))[1][:, :-1])          # the arc 5 -> 4 is missing, 4 -> 5 is there
    big = R.both(257, R.path(257))
    stray = R.both(8, R.path(8))
    graphs = [good[0], asym, good[1], big, good[2], stray, good[3]]
    b = synth.collate(graphs)
    ei = b.edge_index.copy()
    ei[1, b.edge_ptr[5]] = b.node_ptr[4]              # an arc of graph 5 now ends in graph 4
    b = synth.Batch(b.node_ptr, b.edge_ptr, ei)
    vec, val, status, sweeps = run(b, "none")
    assert status.tolist() == [0, dgn.ST_ASYMMETRIC, 0, dgn.ST_TOO_LARGE, 0, dgn.ST_BAD_INDEX, 0]
    ref = run(synth.collate(good), "none")
    rows = np.concatenate([vec[b.node_ptr[g]:b.node_ptr[g + 1]] for g in (0, 2, 4, 6)])
    assert rows.tobytes() == ref[0].tobytes() and val[[0, 2, 4, 6]].tobytes() == ref[1].tobytes(), "a refused graph disturbed the others"
    for g in (1, 3, 5):
        assert (vec[b.node_ptr[g]:b.node_ptr[g + 1]] == 0).all() and np.isnan(val[g]).all() and sweeps[g] == 0
    with pytest.raises(ValueError, match="graph 1 "):
        dgn.laplacian_eigenvectors(synth.collate([good[0], asym]))
    with pytest.raises(ValueError, match="graph 2 has 257 vertices"):
        dgn.laplacian_eigenvectors(synth.collate([good[0], good[1], big]))
    bad = synth.collate([good[0], good[1], stray])
    ei = bad.edge_index.copy()
    ei[0, -1] = bad.num_nodes                          # one past the batch's last vertex
    with pytest.raises(IndexError, match="graph 2 "):
        dgn.laplacian_eigenvectors(synth.Batch(bad.node_ptr, bad.edge_ptr, ei))
    # the loop bound: one sweep is not enough for P9; the graph gets its status, its last iterate, and the call returns
    p9 = synth.collate([R.both(9, R.path(9))])
    vec, val, status, sweeps = run(p9, "none", max_sweeps=1)
    assert status.tolist() == [dgn.ST_NO_CONVERGENCE] and sweeps.tolist() == [1] and np.isfinite(vec).all()
    with pytest.raises(RuntimeError, match="did not converge"):
        dgn.laplacian_eigenvectors(p9, max_sweeps=1)
    assert run(p9, "none")[2].tolist() == [0]


class _NoEigLaunch:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        assert name != "gsn_laplacian_eig_hip", "an empty batch must launch nothing"
        return getattr(self._real, name)


def test_empty_batches_launch_nothing(monkeypatch):
    from gsn_amd import _abi, dgn, synth
    monkeypatch.setattr(_abi, "_lib", _NoEigLaunch(_abi.lib()))
    vec, val, status = dgn.laplacian_eigenvectors(synth.collate([]), check=False, return_values=True)
    assert vec.shape == (0, 4) and val.shape == (0, 4) and status.shape == (0,) and vec.is_cuda
    none = np.zeros((2, 0), dtype=np.int64)
    vec, val = dgn.laplacian_eigenvectors(synth.collate([(0, none), (0, none)]), k=2, return_values=True)
    assert vec.shape == (0, 2) and val.shape == (2, 2) and bool(torch.isnan(val).all())


def test_through_the_model():
    from gsn_amd import dgn, synth
    b = synth.zinc_shape_batch(24, seed=2)
    g = dgn.DGNGraph.from_batch(b, directions=["eig"], norm="none", pos_enc_dim=3)
    assert g.ndata["eig"].shape == (b.num_nodes, 4) and g.ndata["eig"].dtype == torch.float32 and "eig" not in g.edata
    assert torch.equal(g.ndata["pos_enc"], g.ndata["eig"][:, 1:4])
    assert torch.equal(g.ndata["eig"], dgn.laplacian_eigenvectors(b, k=4, norm="none"))
    edge_field = np.random.default_rng(0).integers(0, 3, size=(b.num_edges, 2)).astype(np.float32)
    g2 = dgn.DGNGraph.from_batch(b, directions=["eig", "subgraphs"], edge_field=edge_field)
    assert g2.ndata["eig"].shape == (b.num_nodes, 4) and torch.equal(g2.edata["eig"].cpu(), torch.from_numpy(edge_field))
    g3 = dgn.DGNGraph.from_batch(b, directions=["subgraphs", "eig", "edge_feat"], node_field=edge_field[:b.num_nodes, :1], edge_feat=edge_field,
                                 norm="sym")
    assert g3.ndata["eig"].shape == (b.num_nodes, 5) and torch.equal(g3.ndata["eig"][:, 1:], dgn.laplacian_eigenvectors(b, norm="sym"))
    assert g3.edata["eig"].shape == (b.num_edges, 2)
    # positional_encoding twice: 8 columns, as HIV.py:49 concatenates
    assert dgn.positional_encoding(g, 4, "none") is g and g.ndata["eig"].shape == (b.num_nodes, 8)
    assert torch.equal(g.ndata["eig"][:, :4], g.ndata["eig"][:, 4:])
    # a DGN over the eigenvector field: forward and backward, finite
    g = dgn.DGNGraph.from_batch(b, directions=["eig"], norm="none", pos_enc_dim=3)
    torch.manual_seed(0)
    net = dgn.DGNNet(dict(L=2, hidden_dim=16, out_dim=16, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0,
                          dropout=0.0, graph_norm=False, batch_norm=True, aggregators="mean dir1-av dir2-dx", scalers="identity", towers=5,
                          divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1, posttrans_layers=1, pos_enc_dim=3,
                          device="cuda", avg_d={"log": 1.0})).to("cuda").train()
    dims = [119, 4, 12, 12, 10, 6, 6, 2, 2]
    rng = np.random.default_rng(1)
    codes = torch.from_numpy(np.stack([rng.integers(0, d, size=b.num_nodes) for d in dims], axis=1)).to("cuda")
    scores = net(g, codes, None, g.snorm_n, None)
    assert scores.shape == (b.num_graphs, 1) and bool(torch.isfinite(scores).all())
    net.loss(scores, torch.from_numpy(rng.integers(0, 2, size=b.num_graphs)).float().to("cuda")).backward()
    grads = [p.grad for p in net.parameters()]
    assert all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
    assert float(net.embedding_pos_enc.weight.grad.abs().max()) > 0
