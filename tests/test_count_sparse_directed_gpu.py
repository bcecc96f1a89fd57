"""Directed plans on the sparse counting kernel (gsn_count_sparse_hip, csrc/count_sparse.hip) on the GPU: digraphs the LDS-resident kernel
refuses, against the oracle, the reference's goldens and the LDS kernel, and the routes that lead there (count_batch large="sparse",
prepare_graphs, the per-graph drop-ins).  Integer work: every comparison is bit-exact."""
import numpy as np
import pytest
import torch

from helpers import case_names, count_case, directed_patterns

pytestmark = pytest.mark.gpu

UND = [[(0, 1), (1, 2), (2, 0)], [(i, (i + 1) % 6) for i in range(6)], [(0, 1), (0, 2), (0, 3)], [(0, 1), (1, 2), (2, 3)]]
BOTH = [el + [(v, u) for u, v in el] for el in UND]


def _patterns():
    return [el for el, _, _ in directed_patterns()]


def _digraph(seed, n, m, loops=0, dups=0, extra=None):
    """m random arcs without self loops (after those of `extra`), `dups` of them repeated, `loops` self loops, shuffled."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=m)
    dst = (src + rng.integers(1, n, size=m)) % n
    ei = np.stack([src, dst]).astype(np.int64)
    if extra is not None:
        ei = np.concatenate([extra, ei], axis=1)
    lv = rng.integers(0, n, size=loops)
    ei = np.concatenate([ei, ei[:, :dups], np.stack([lv, lv])], axis=1)
    return n, np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def _hub(seed, n, n_out, n_in, n_random):
    rng = np.random.default_rng(seed)
    spokes = rng.choice(np.arange(1, n), size=n_out + n_in, replace=False)
    out_arcs = np.stack([np.zeros(n_out, np.int64), spokes[:n_out]])
    in_arcs = np.stack([spokes[n_out:], np.zeros(n_in, np.int64)])
    return _digraph(seed + 1, n, n_random, extra=np.concatenate([out_arcs, in_arcs], axis=1).astype(np.int64))


def large_digraphs(induced):
    """The hub has 500 out- and 300 in-spokes for the non-induced plans.  Induced plans have no closed-form tail for the leaves of a star (each
    leaf names the others in its non-adjacency masks), so ONE lane enumerates the ~d^3 / 6 leaf triples of the hub's own cell by itself: 215 s
    on an MI355X at 500 / 300.  The induced batch therefore carries the hub with 100 / 60 spokes; everything else is the same."""
    spokes = (100, 60) if induced else (500, 300)
    return [_digraph(1, 769, 3000, loops=3, dups=11), _digraph(2, 1000, 5000), _digraph(3, 900, 9000), _hub(4, 1200, spokes[0], spokes[1], 2500),
            _digraph(5, 40, 110, loops=1, dups=3), (5, np.zeros((2, 0), np.int64))]


_BATCH = {}


def _batch(induced):
    from gsn_amd import synth
    if induced not in _BATCH:
        _BATCH[induced] = synth.collate(large_digraphs(induced))
    return _BATCH[induced]


def _local(b):
    return b.edge_index - np.repeat(b.node_ptr[:-1], np.diff(b.edge_ptr))[None, :]


_ORACLE = {}


def _oracle(induced):
    """The oracle's identifiers of the digraph patterns on the batch, computed once per `induced` and never written to."""
    from oracle import oracle
    b = _batch(induced)
    if induced not in _ORACLE:
        ref = oracle.counts2ids("vertex", induced, b.node_ptr, b.edge_ptr, _local(b), _patterns(), n_threads=8, directed=True)
        ref.setflags(write=False)
        _ORACLE[induced] = ref
    return _ORACLE[induced]


def _oracle_one(n, ei, pats, induced=False):
    from oracle import oracle
    return oracle.counts2ids("vertex", induced, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats, n_threads=8, directed=True)


@pytest.mark.parametrize("induced", [False, True])
def test_large_directed_batch_matches_oracle(induced):
    """(a) one collated batch of digraphs the LDS kernel refuses (769, 1 000 and 900 vertices, a hub of 1 200 vertices: large_digraphs), one
    it would take and one without arcs, counted in one launch of the sparse kernel."""
    from gsn_amd.counting import counts2ids_batch
    got = counts2ids_batch(_batch(induced), _patterns(), "vertex", induced, directed=True, large="sparse").cpu().numpy()
    ref = _oracle(induced)
    assert got.shape == ref.shape
    assert ref.sum() > 0
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("name", case_names("counts_directed"))
def test_goldens_forced_onto_the_sparse_kernel(name):
    """(b) stating max_nodes = 769 sends the small digraphs of the goldens straight to the sparse kernel."""
    from gsn_amd.counting import CountPlan, count_batch
    c = count_case(name, "counts_directed")
    plan = CountPlan.get(c["patterns"], "vertex", c["induced"], False, directed=True)
    out, st = count_batch(plan, c["node_ptr"], c["edge_ptr"], c["edge_index_local"], ids_are_global=False, max_nodes=769,
                          max_edges=int(np.diff(c["edge_ptr"]).max()), large="sparse")
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(out.cpu().numpy(), c["counts"])


@pytest.mark.parametrize("induced", [False, True])
def test_sparse_kernel_agrees_with_the_lds_kernel(induced):
    """(c) digraphs of 64, 300 and 700 vertices with repeated arcs and self loops on both kernels."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    b = synth.collate([_digraph(11, 64, 400, loops=4, dups=9), _digraph(12, 300, 1300, loops=2, dups=5), _digraph(13, 700, 2800, loops=3, dups=20)])
    plan = CountPlan.get(_patterns(), "vertex", induced, False, directed=True)
    lds, st_l = count_batch(plan, b.node_ptr, b.edge_ptr, b.edge_index, large="refuse")
    sp, st_s = count_batch(plan, b.node_ptr, b.edge_ptr, b.edge_index, max_nodes=769, max_edges=int(np.diff(b.edge_ptr).max()), large="sparse")
    assert int(lds.sum().item()) > 0
    assert torch.equal(sp, lds) and torch.equal(st_s, st_l)


def test_symmetric_digraph_equals_undirected_plan():
    """(d) a molecule-shaped graph of 1 000 vertices with both arcs of every edge, bidirected patterns: the undirected plan's counts."""
    from gsn_amd import synth
    from gsn_amd.counting import counts2ids_batch
    n, ei = synth.zinc_shape_graph(np.random.default_rng(5), mean_n=1000, sd_n=0.0, n_min=1000, n_max=1000, ring_rate=1000 / 16.0)
    assert n == 1000
    b = synth.collate([(n, ei)])
    for induced in (False, True):
        a = counts2ids_batch(b, UND, "vertex", induced, large="sparse")
        d = counts2ids_batch(b, BOTH, "vertex", induced, directed=True, large="sparse")
        assert torch.equal(a, d) and int(a.sum()) > 0


def test_graph_ids_subset_leaves_other_rows():
    """(e) a subset of the graphs into the caller's `out`: the rows of the others keep what they held."""
    from gsn_amd.counting import CountPlan, count_batch
    batch, ref = _batch(False), _oracle(False)
    plan = CountPlan.get(_patterns(), "vertex", False, False, directed=True)
    out = torch.full(ref.shape, -7, dtype=torch.int64, device="cuda")
    ids = [4, 1, 5]
    count_batch(plan, batch.node_ptr, batch.edge_ptr, batch.edge_index, out=out, graph_ids=ids, large="sparse")
    want = np.full(ref.shape, -7, dtype=np.int64)
    for g in ids:
        want[batch.node_ptr[g]:batch.node_ptr[g + 1]] = ref[batch.node_ptr[g]:batch.node_ptr[g + 1]]
    assert np.array_equal(out.cpu().numpy(), want)


def test_bad_index_zeroes_its_graph_only():
    """(e) a column pointing past the batch: GSN_ST_BAD_INDEX and zero rows for that graph, the other graph counted."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    n, ei = _digraph(21, 800, 4000)
    pats = _patterns()[:3]
    ref = _oracle_one(n, ei, pats)
    assert ref.sum() > 0
    b = synth.collate([(n, ei), (n, ei)])
    plan = CountPlan.get(pats, "vertex", False, False, directed=True)
    bad = b.edge_index.copy()
    bad[1, 5] = 2 * n
    out, st = count_batch(plan, b.node_ptr, b.edge_ptr, bad, check=False, large="sparse")
    assert st.cpu().tolist() == [3, 0]
    assert not out[:n].any().item() and np.array_equal(out[n:].cpu().numpy(), ref)
    with pytest.raises(ValueError, match="vertex id"):
        count_batch(plan, b.node_ptr, b.edge_ptr, bad, large="sparse")


def test_prepare_graphs_and_drop_ins_route_large_digraphs():
    """(f) prepare_graphs on digraphs of 900, 20 and 300 vertices: the oracle's identifiers, in the caller's order; the per-graph drop-ins on
    800 vertices; the edge counter still refuses directed work."""
    from types import SimpleNamespace
    from gsn_amd import counting, dataset, patterns
    graphs = [_digraph(31, 900, 3000, dups=7), _digraph(32, 20, 60, dups=2), _digraph(33, 300, 1000, dups=4)]
    pats = _patterns()[:4]
    dicts = []
    for el in pats:
        sg, part, memb, aut = patterns.automorphism_orbits(edge_list=el, print_msgs=False, directed=True, directed_orbits=False)
        dicts.append({"subgraph": sg, "orbit_partition": part, "orbit_membership": memb, "aut_count": aut})
    recs = [SimpleNamespace(edge_mat=torch.from_numpy(ei), node_features=torch.zeros(n, 1), label=0) for n, ei in graphs]
    prepared = dataset.prepare_graphs(recs, dicts, {"induced": False, "directed": True}, False, "synthetic", "vertex")
    for (n, ei), d in zip(graphs, prepared):
        ref = _oracle_one(n, ei, pats)
        assert ref.sum() > 0
        assert np.array_equal(d.identifiers.numpy(), ref) and d.graph_size == n

    n, ei = _digraph(34, 800, 3200, dups=6)
    ref = _oracle_one(n, ei, pats)
    got = counting.subgraph_isomorphism_vertex_counts(torch.from_numpy(ei), subgraph_dict=dicts[0], induced=False, num_nodes=n, directed=True)
    w = len(dicts[0]["orbit_partition"])
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), ref[:, :w].astype(np.float64))

    class Data:
        pass
    data = Data()
    data.x = torch.ones(n, 1)
    data.edge_index = torch.from_numpy(ei)
    res = counting.subgraph_counts2ids(counting.subgraph_isomorphism_vertex_counts, data, dicts, {"induced": False, "directed": True})
    assert res.identifiers.dtype == torch.int64 and np.array_equal(res.identifiers.numpy(), ref)
    with pytest.raises(NotImplementedError):
        counting.subgraph_counts2ids(counting.subgraph_isomorphism_edge_counts, data, dicts, {"induced": False, "directed": True})
    with pytest.raises(NotImplementedError):
        counting.subgraph_isomorphism_edge_counts(torch.from_numpy(ei), subgraph_dict=dicts[0], induced=False, directed=True)
    with pytest.raises(NotImplementedError):
        dataset.prepare_graphs(recs, dicts, {"induced": False, "directed": True}, False, "synthetic", "edge")


def test_default_still_refuses_large_digraphs():
    """(g) without `large` nothing changes."""
    from gsn_amd import _abi, synth
    from gsn_amd.counting import counts2ids_batch
    b = synth.collate([_digraph(41, 800, 3000)])
    with pytest.raises(_abi.GsnError, match="768"):
        counts2ids_batch(b, _patterns(), "vertex", False, directed=True)
