"""Wide counting plans (pattern lists whose largest pattern has 10 .. 16 vertices) on the GPU: the wide instantiation of the sparse kernel
(csrc/count_sparse.hip: sparse_search_kernel<DIR, true>) against the oracle, and the routes that lead to it -- count_batch with
large="sparse", the per-graph drop-ins, dataset.prepare_graphs.  Every test that builds a wide plan fails on a build without them: the
plan compiler answers "k <= 9"."""
from types import SimpleNamespace

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _el(g):
    return [(int(u), int(v)) for u, v in nx.convert_node_labels_to_integers(g).edges]


def _cycles(lo, hi):
    return [_el(nx.cycle_graph(k)) for k in range(lo, hi + 1)]


def _graph(g):
    g = nx.convert_node_labels_to_integers(g)
    e = np.array(list(g.edges), dtype=np.int64).reshape(-1, 2).T
    return g.number_of_nodes(), np.ascontiguousarray(np.concatenate([e, e[::-1]], axis=1))


PLANS = {"mixed3_12": _cycles(3, 12),
         "long": _cycles(13, 16) + [_el(nx.path_graph(10)), _el(nx.binomial_tree(4))]}


def _zinc769():
    from gsn_amd import synth
    n, ei = synth.zinc_shape_graph(np.random.default_rng(769), mean_n=769, sd_n=0.0, n_min=769, n_max=769, ring_rate=40.0)
    assert n == 769
    return n, ei


@pytest.fixture(scope="module")
def batch():
    """ladder, grid, circular ladder, two cycles as targets, a graph smaller than every wide pattern, an edge-less graph, eight molecules"""
    from gsn_amd import synth
    z = synth.zinc_shape_batch(8, seed=7)
    graphs = [_graph(nx.ladder_graph(8)), _graph(nx.grid_2d_graph(3, 6)), _graph(nx.circular_ladder_graph(9)), _graph(nx.cycle_graph(12)),
              _graph(nx.cycle_graph(16)), _graph(nx.path_graph(4)), (5, np.zeros((2, 0), dtype=np.int64))] + [z.graph(g) for g in range(z.num_graphs)]
    return synth.collate(graphs)


def _local(b):
    return b.edge_index - np.repeat(b.node_ptr[:-1], np.diff(b.edge_ptr))[None, :]


_ORACLE = {}


def _oracle(b, name, mode, induced):
    """The oracle's identifiers of PLANS[name] on the batch, computed once per (plan, mode, induced) and never written to."""
    from oracle import oracle
    key = (name, mode, induced)
    if key not in _ORACLE:
        ref = oracle.counts2ids(mode, induced, b.node_ptr, b.edge_ptr, _local(b), PLANS[name], n_threads=8)
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
@pytest.mark.parametrize("name", ["mixed3_12", "long"])
def test_batch_matches_oracle(batch, name, mode, induced):
    """One launch of the wide instantiation over the batch, with batch-global and with graph-local vertex ids."""
    from gsn_amd.counting import CountPlan, count_batch
    plan = CountPlan.get(PLANS[name], mode, induced, wide=True)
    assert plan.wide
    ref = _oracle(batch, name, mode, induced)
    got, st = count_batch(plan, batch.node_ptr, batch.edge_ptr, batch.edge_index, ids_are_global=True, large="sparse")
    assert got.shape == ref.shape and not st.any().item()
    assert np.array_equal(got.cpu().numpy(), ref)
    got_l, _ = count_batch(plan, batch.node_ptr, batch.edge_ptr, _local(batch), ids_are_global=False, large="sparse")
    assert np.array_equal(got_l.cpu().numpy(), ref)
    assert ref[:, 7:].sum() > 0 if name == "mixed3_12" else ref.sum() > 0      # (columns 7 ..: the cycles of 10, 11 and 12 vertices)


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
def test_small_patterns_of_a_wide_table_equal_the_lds_kernel(batch, mode, induced):
    """The columns of the <= 9-vertex patterns of the mixed table are bit-equal to what the narrow plan gives on the LDS-resident kernel."""
    from gsn_amd.counting import CountPlan, count_batch, counts2ids_batch
    narrow = counts2ids_batch(batch, _cycles(3, 9), mode, induced)
    plan = CountPlan.get(PLANS["mixed3_12"], mode, induced, wide=True)
    got, _ = count_batch(plan, batch.node_ptr, batch.edge_ptr, batch.edge_index, large="sparse")
    assert narrow.shape[1] == 7 and int(narrow.sum().item()) > 0
    assert torch.equal(got[:, :7], narrow)


@pytest.mark.parametrize("mode", ["vertex", "edge"])
def test_769_vertices(mode):
    from gsn_amd.counting import CountPlan, count_batch
    from oracle import oracle
    n, ei = _zinc769()
    pats = [_el(nx.cycle_graph(10)), _el(nx.cycle_graph(12)), _el(nx.path_graph(10))]
    for induced in (False, True):
        plan = CountPlan.get(pats, mode, induced, wide=True)
        got, _ = count_batch(plan, [0, n], [0, ei.shape[1]], ei, ids_are_global=False, max_nodes=n, max_edges=ei.shape[1], large="sparse")
        ref = oracle.counts2ids(mode, induced, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats, n_threads=8)
        assert ref.sum() > 0 and np.array_equal(got.cpu().numpy(), ref)


def test_directed_wide_plan():
    """A directed 10-cycle and a directed 12-path in a digraph that holds both under random arcs, and in one that holds them induced."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    from oracle import oracle
    pats = [[(i, (i + 1) % 10) for i in range(10)], [(i, i + 1) for i in range(11)]]
    rng = np.random.default_rng(5)
    arcs = [(i, i + 1) for i in range(14)] + [(9, 0)] + [(int(a), int(b)) for a, b in rng.integers(0, 15, size=(9, 2)) if a != b]
    arcs2 = [(i, (i + 1) % 10) for i in range(10)] + [(10, 0), (5, 11)] + [(12 + i, 13 + i) for i in range(12)]
    b = synth.collate([(15, np.array(arcs, dtype=np.int64).T), (25, np.array(arcs2, dtype=np.int64).T)])
    for induced in (False, True):
        plan = CountPlan.get(pats, "vertex", induced, False, True, wide=True)
        assert plan.wide and plan.directed
        got, _ = count_batch(plan, b.node_ptr, b.edge_ptr, b.edge_index, large="sparse")
        ref = oracle.counts2ids("vertex", induced, b.node_ptr, b.edge_ptr, _local(b), pats, n_threads=8, directed=True)
        assert (ref.sum(0) > 0).all() and np.array_equal(got.cpu().numpy(), ref)


def test_statuses_leave_other_rows_intact():
    """A graph whose matches use a column without its reverse (KeyError) and one with an endpoint outside it (bad index), inside a batch."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    from oracle import oracle
    pats = PLANS["mixed3_12"]
    lad, grid = _graph(nx.ladder_graph(8)), _graph(nx.grid_2d_graph(3, 6))
    cut = (lad[0], np.delete(lad[1], 0, axis=1))                     # (every ladder edge lies on a 4-cycle)
    b = synth.collate([lad, cut, grid, grid])
    bad = b.edge_index.copy()
    bad[1, b.edge_ptr[2] + 3] = b.num_nodes + 9
    plan = CountPlan.get(pats, "edge", False, wide=True)
    out, st = count_batch(plan, b.node_ptr, b.edge_ptr, bad, check=False, large="sparse")
    assert st.cpu().tolist() == [0, 1, 3, 0]
    out = out.cpu().numpy()
    for g, (n, ei) in ((0, lad), (3, grid)):
        ref = oracle.counts2ids("edge", False, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats, n_threads=8)
        assert ref.sum() > 0 and np.array_equal(out[b.edge_ptr[g]:b.edge_ptr[g + 1]], ref)
    assert not out[b.edge_ptr[2]:b.edge_ptr[3]].any()
    with pytest.raises(KeyError):
        count_batch(plan, b.node_ptr[:3], b.edge_ptr[:3], b.edge_index[:, :b.edge_ptr[2]], large="sparse")


def test_refusals_before_any_launch(batch):
    from gsn_amd import _abi
    from gsn_amd.counting import CountPlan, count_batch, count_batch_side
    plan = CountPlan.get(PLANS["mixed3_12"], "edge", False, wide=True)
    with pytest.raises(_abi.GsnError, match='large="sparse"'):
        count_batch(plan, batch.node_ptr, batch.edge_ptr, batch.edge_index)
    with pytest.raises(ValueError, match="wide plans count only"):
        count_batch(plan, batch.node_ptr, batch.edge_ptr, batch.edge_index, encode=([3] * plan.n_cols, True))
    with pytest.raises(ValueError, match="wide plans count only"):
        count_batch_side(plan, None, None, None, 1, 1)
    # the LDS kernel's entry, handed the table all the same, names the kernel that takes it
    dev = torch.device("cuda")
    npt, ept = (torch.as_tensor(x, device=dev) for x in (batch.node_ptr, batch.edge_ptr))
    ei = torch.as_tensor(batch.edge_index, device=dev)
    out = torch.zeros((batch.num_edges, plan.n_cols), dtype=torch.int64, device=dev)
    st = torch.zeros(batch.num_graphs, dtype=torch.int32, device=dev)
    rc = _abi.lib().gsn_count_hip(_abi.ptr(plan.table), plan.device_table(dev).data_ptr(), len(plan.table), batch.num_graphs, npt.data_ptr(),
                                  ept.data_ptr(), ei.data_ptr(), ei.stride(0), 1, None, batch.num_graphs, 64, 256, out.data_ptr(), st.data_ptr(),
                                  _abi.current_stream())
    assert rc == -2
    with pytest.raises(_abi.GsnError, match="wide plan .*gsn_count_sparse_hip only"):
        _abi.check(rc, "gsn_count_hip")


def test_drop_ins_and_prepare_graphs_with_cycles_up_to_12():
    """--id_type cycle_graph --k 12 through the drop-in modules: prepare_graphs over a dozen graphs of mixed sizes (the 769-vertex one among
    them) and the per-graph functions equal the oracle; downgrade_k to 8 equals a fresh k = 8 preparation."""
    from gsn_amd import counting, dataset, patterns, synth
    from oracle import oracle
    z = synth.zinc_shape_batch(6, seed=3)
    graphs = [_graph(nx.ladder_graph(8)), _graph(nx.circular_ladder_graph(9)), _zinc769(), _graph(nx.cycle_graph(12)), synth.er_graph(70, 90, 2),
              synth.er_graph(300, 330, 4)] + [z.graph(g) for g in range(6)]
    pats = _cycles(3, 12)

    def dicts_of(fn, pats):
        import contextlib, io
        out = []
        with contextlib.redirect_stdout(io.StringIO()):
            for el in pats:
                sg, part, memb, aut = fn(edge_list=el, directed=False, directed_orbits=False)
                out.append({"subgraph": sg, "orbit_partition": part, "orbit_membership": memb, "aut_count": aut})
        return out

    recs = [SimpleNamespace(edge_mat=torch.from_numpy(ei), node_features=torch.zeros(n, 1), label=0) for n, ei in graphs]
    params = {"induced": False, "directed": False}
    for mode, fn, count_fn in (("vertex", patterns.automorphism_orbits, counting.subgraph_isomorphism_vertex_counts),
                               ("edge", patterns.induced_edge_automorphism_orbits, counting.subgraph_isomorphism_edge_counts)):
        dicts = dicts_of(fn, pats)
        refs = [oracle.counts2ids(mode, False, np.array([0, n]), np.array([0, ei.shape[1]]), ei, pats, n_threads=8) for n, ei in graphs]
        assert sum(int(r[:, 7:].sum()) for r in refs) > 0
        prepared = dataset.prepare_graphs(recs, dicts, params, False, "synthetic", mode)
        for (n, ei), d, ref in zip(graphs, prepared, refs):
            assert np.array_equal(d.identifiers.numpy(), ref) and d.graph_size == n
        sizes = [len(d["orbit_partition"]) for d in dicts]
        down, kept = dataset.downgrade_k(prepared, 8, sizes, 3)
        fresh = dataset.prepare_graphs(recs, dicts[:6], params, False, "synthetic", mode)
        assert kept == sizes[:6]
        for a, b in zip(down, fresh):
            assert torch.equal(a.identifiers, b.identifiers)
        # the per-graph signatures of the reference: one pattern (the 12-cycle), and all patterns through subgraph_counts2ids
        for g in (1, 2, 3):
            n, ei = graphs[g]
            one = count_fn(torch.from_numpy(ei), subgraph_dict=dicts[-1], induced=False, num_nodes=n)
            assert one.dtype == torch.float64 and np.array_equal(one.numpy(), refs[g][:, -1:].astype(np.float64))
            data = SimpleNamespace(edge_index=torch.from_numpy(ei), x=torch.zeros(n, 1))
            counting.subgraph_counts2ids(count_fn, data, dicts, params)
            assert np.array_equal(data.identifiers.numpy(), refs[g])
