"""The sparse counting kernel (gsn_count_sparse_hip, csrc/count_sparse.hip) on the GPU: graphs the LDS-resident kernel refuses, against
the oracle and against the LDS kernel, and the routes that lead to it (count_batch large="sparse", prepare_graphs, the per-graph drop-ins)."""
import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cycles(lo, hi):
    return [list(nx.cycle_graph(k).edges) for k in range(lo, hi + 1)]


def _cliques(lo, hi):
    return [list(nx.complete_graph(k).edges) for k in range(lo, hi + 1)]


PATTERNS = _cycles(3, 5) + _cliques(3, 4)


def _zinc(n, seed):
    from gsn_amd import synth
    got, ei = synth.zinc_shape_graph(np.random.default_rng(seed), mean_n=n, sd_n=0.0, n_min=n, n_max=n, ring_rate=n / 16.0)
    assert got == n
    return got, ei


def _clique_union(n, n_cliques, seed):
    from gsn_amd import synth
    rng = np.random.default_rng(seed)
    und = set()
    for _ in range(n_cliques):
        vs = np.sort(rng.choice(n, size=int(rng.integers(8, 22)), replace=False))
        und.update((int(a), int(b)) for i, a in enumerate(vs) for b in vs[i + 1:])
    return n, synth.undirected_to_edge_index(n, sorted(und))


def _hub(n, n_spokes, n_random, seed):
    from gsn_amd import synth
    rng = np.random.default_rng(seed)
    und = {(0, int(v)) for v in rng.choice(np.arange(1, n), size=n_spokes, replace=False)}
    while len(und) < n_spokes + n_random:
        a, b = (int(x) for x in rng.integers(1, n, size=2))
        if a != b:
            und.add((min(a, b), max(a, b)))
    return n, synth.undirected_to_edge_index(n, sorted(und))


def large_graphs():
    from gsn_amd import synth
    return [_zinc(769, 1), _zinc(1000, 2), _clique_union(900, 14, 3), _hub(1200, 800, 1500, 4), synth.er_graph(800, 1000, 1), synth.er_graph(40, 90, 5)]


@pytest.fixture(scope="module")
def batch():
    from gsn_amd import synth
    return synth.collate(large_graphs())


def _local(b):
    return b.edge_index - np.repeat(b.node_ptr[:-1], np.diff(b.edge_ptr))[None, :]


_ORACLE = {}


def _oracle(b, mode, induced):
    """The oracle's identifiers of PATTERNS on the batch, computed once per (mode, induced) and never written to."""
    from oracle import oracle
    key = (mode, induced)
    if key not in _ORACLE:
        ref = oracle.counts2ids(mode, induced, b.node_ptr, b.edge_ptr, _local(b), PATTERNS, n_threads=8)
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
def test_large_batch_matches_oracle(batch, mode, induced):
    """(a) one collated batch of graphs the LDS kernel refuses (769 and 1 000 vertices, clique unions, a hub of degree 800) and one it would
    take, counted in one launch of the sparse kernel."""
    from gsn_amd.counting import counts2ids_batch
    got = counts2ids_batch(batch, PATTERNS, mode, induced, large="sparse").cpu().numpy()
    ref = _oracle(batch, mode, induced)
    assert got.shape == ref.shape
    assert ref.sum() > 0
    assert np.array_equal(got, ref)


@pytest.fixture(scope="module")
def many():
    from gsn_amd import synth
    return synth.zinc_shape_batch(3000, seed=11)


@pytest.mark.parametrize("mode,pats", [("edge", _cycles(3, 6)), ("vertex", [list(nx.star_graph(k).edges) for k in (3, 4)])])
def test_one_graph_of_more_than_65535_vertices_and_columns(many, mode, pats):
    """(b) 3 000 molecule-shaped graphs as ONE graph (node_ptr = [0, N]) on the sparse kernel against the same graphs as a batch on the LDS
    kernel: the patterns are connected, so every row is the same."""
    from gsn_amd.counting import CountPlan, count_batch, counts2ids_batch
    b = many
    assert b.num_nodes > 65535 and b.num_edges > 65535
    ref = counts2ids_batch(b, pats, mode, False)
    plan = CountPlan.get(pats, mode, False)
    got, st = count_batch(plan, [0, b.num_nodes], [0, b.num_edges], b.edge_index, ids_are_global=True, max_nodes=b.num_nodes,
                          max_edges=b.num_edges, large="sparse")
    assert int(ref.sum().item()) > 0
    assert torch.equal(got, ref)
    assert st.cpu().tolist() == [0]


def test_graph_ids_subset_leaves_other_rows(batch):
    """(c) a subset of the graphs into the caller's `out`: the rows of the others keep what they held."""
    from gsn_amd.counting import CountPlan, count_batch
    for mode in ("vertex", "edge"):
        ref = _oracle(batch, mode, False)
        plan = CountPlan.get(PATTERNS, mode, False)
        out = torch.full(ref.shape, -7, dtype=torch.int64, device="cuda")
        ids = [4, 1, 5]
        count_batch(plan, batch.node_ptr, batch.edge_ptr, batch.edge_index, out=out, graph_ids=ids, large="sparse")
        ptr = batch.node_ptr if mode == "vertex" else batch.edge_ptr
        want = np.full(ref.shape, -7, dtype=np.int64)
        for g in ids:
            want[ptr[g]:ptr[g + 1]] = ref[ptr[g]:ptr[g + 1]]
        assert np.array_equal(out.cpu().numpy(), want)


def test_statuses_on_800_vertices():
    """(d) an endpoint outside its graph zeroes that graph only (GSN_ST_BAD_INDEX); a triangle on a column whose reverse is no column is
    the reference's KeyError."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    from oracle import oracle
    n, ei = synth.er_graph(800, 4000, 2)
    pats = _cycles(3, 3)
    b = synth.collate([(n, ei), (n, ei)])
    ref = oracle.counts2ids("edge", False, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats, n_threads=8)
    assert ref.sum() > 0
    plan = CountPlan.get(pats, "edge", False)
    bad = b.edge_index.copy()
    bad[1, 5] = 2 * n                                     # (a column of the first graph pointing past the batch)
    out, st = count_batch(plan, b.node_ptr, b.edge_ptr, bad, check=False, large="sparse")
    assert st.cpu().tolist() == [3, 0]
    E = ei.shape[1]
    assert not out[:E].any().item() and np.array_equal(out[E:].cpu().numpy(), ref)
    with pytest.raises(ValueError, match="vertex id"):
        count_batch(plan, b.node_ptr, b.edge_ptr, bad, large="sparse")
    c = int(np.nonzero(ref[:, 0])[0][0])
    rev = int(np.nonzero((ei[0] == ei[1, c]) & (ei[1] == ei[0, c]))[0][0])
    cut = np.delete(ei, rev, axis=1)
    with pytest.raises(KeyError):
        count_batch(plan, [0, n], [0, cut.shape[1]], cut, ids_are_global=False, large="sparse")


def test_prepare_graphs_and_drop_ins_route_large_graphs():
    """(e) prepare_graphs on graphs of 20, 300 and 900 vertices: the oracle's identifiers, in the caller's order; the per-graph drop-in on
    800 vertices."""
    from types import SimpleNamespace
    from gsn_amd import counting, dataset, patterns, synth
    from oracle import oracle
    graphs = [synth.er_graph(900, 1500, 7), synth.er_graph(20, 40, 8), synth.er_graph(300, 600, 9)]
    pats = _cycles(3, 4)
    dicts = []
    for el in pats:
        sg, part, memb, aut = patterns.automorphism_orbits(edge_list=el, directed=False, directed_orbits=False)
        dicts.append({"subgraph": sg, "orbit_partition": part, "orbit_membership": memb, "aut_count": aut})
    recs = [SimpleNamespace(edge_mat=torch.from_numpy(ei), node_features=torch.zeros(n, 1), label=0) for n, ei in graphs]
    prepared = dataset.prepare_graphs(recs, dicts, {"induced": False, "directed": False}, False, "synthetic", "vertex")
    for (n, ei), d in zip(graphs, prepared):
        ref = oracle.counts2ids("vertex", False, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats, n_threads=8)
        assert np.array_equal(d.identifiers.numpy(), ref) and d.graph_size == n
    n, ei = synth.er_graph(800, 1000, 1)
    got = counting.subgraph_isomorphism_vertex_counts(torch.from_numpy(ei), subgraph_dict=dicts[0], induced=False, num_nodes=n)
    ref = oracle.counts2ids("vertex", False, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats[:1], n_threads=8)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), ref.astype(np.float64))


def test_default_still_refuses_and_encodings_stay_on_the_lds_kernel():
    """(f) without `large` nothing changes; the fused encodings are not offered by the sparse kernel."""
    from gsn_amd import _abi, synth
    from gsn_amd.counting import CountPlan, count_batch, counts2ids_batch
    b = synth.collate([synth.er_graph(800, 1000, 1)])
    with pytest.raises(_abi.GsnError, match="768"):
        counts2ids_batch(b, _cycles(3, 3), "vertex", False)
    plan = CountPlan.get(_cycles(3, 3), "vertex", False)
    with pytest.raises(ValueError, match="sparse"):
        count_batch(plan, b.node_ptr, b.edge_ptr, b.edge_index, encode=([3], True), large="sparse")
