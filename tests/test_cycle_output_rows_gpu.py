"""The cycle instantiation's output rows and set-up on the headline step's flag combination (count.hip: CycKeys -- one loop over rows
writes the int64 row as two 16-byte stores and the 2-byte identifier mask from one 8-byte LDS read; 16-byte LDS clears; no LDS atomic for
the vertex count and the bad-index flag) and on the generic combination (CycAny, the row-pack launch of count_batch_side).  Every case
runs through CountLayerStep (keys) and count_batch_side (packs) and is compared to oracle.counts2ids on the CPU: int64 identifiers,
identifier masks / pack columns (= the one-hot of the clamped or unclamped class as bits) and status words, all exactly."""
import networkx as nx
import numpy as np
import pytest
import torch

from step_keys_batches import make_layer

pytestmark = pytest.mark.gpu
CYCLES = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
ST_KEYERROR, ST_TOO_LARGE, ST_BAD_INDEX = 1, 2, 3
_ORACLE = {}


def _both(und):
    und = np.asarray(und, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([und.T, und.T[::-1]], axis=1)


def _oracle(n, ei):
    """oracle.counts2ids of one graph (graph-local ids), computed once per distinct graph of the module."""
    from oracle import oracle
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    key = (n, ei.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = oracle.counts2ids("edge", False, np.array([0, n], np.int64), np.array([0, ei.shape[1]], np.int64), ei, CYCLES, n_threads=8)
    return _ORACLE[key]


def _random_graph(seed, n, m, loops=0):
    """m undirected pairs among n vertices, both directions, + `loops` self-loop columns (rows that carry nothing: zero)."""
    rng = np.random.default_rng(seed)
    pairs = [(u, v) for u in range(n) for v in range(u + 1, n)]
    ei = _both([pairs[i] for i in rng.permutation(len(pairs))[:m]])
    if loops:
        ei = np.concatenate([ei, np.tile(np.arange(loops, dtype=np.int64), (2, 1))], axis=1)
    return n, ei


def _ring(n, chords=()):
    return n, _both([(i, (i + 1) % n) for i in range(n)] + list(chords))


def _collate(graphs, ids_are_global):
    node_ptr, edge_ptr, cols = [0], [0], []
    for n, ei in graphs:
        cols.append(np.asarray(ei, dtype=np.int64).reshape(2, -1) + (node_ptr[-1] if ids_are_global else 0))
        node_ptr.append(node_ptr[-1] + n); edge_ptr.append(edge_ptr[-1] + cols[-1].shape[1])
    return np.asarray(node_ptr, np.int64), np.asarray(edge_ptr, np.int64), np.ascontiguousarray(np.concatenate(cols, 1))


def _hot_bits(ids, classes, clamp):
    """Per row: bit (first column of c's classes + class) of every column c whose count has a class."""
    m, first = np.zeros(ids.shape[0], dtype=np.int64), 0
    for c, ncls in enumerate(classes):
        cls = np.minimum(ids[:, c], ncls - 1) if clamp else ids[:, c]
        ok = cls < ncls
        m[ok] |= 1 << (first + cls[ok])
        first += ncls
    return m


@pytest.fixture(scope="module")
def layer():
    return make_layer("source_to_target", seed=1)


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")      # (read at every launch: the library names the instantiation it takes on stderr)


def _check(capfd, layer, graphs, want_ids, want_status, blank=(), classes=(3, 3, 3, 3), clamp=True, ids_are_global=True, max_nodes=None,
           max_edges=None, misaligned=False):
    """The collated graphs through the key step and through the row-pack launch.  ``blank``: graphs that are reported, not counted (zero
    identifiers, no class bit); ``misaligned``: the int64 rows start 8 bytes behind a 16-byte boundary."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan, count_batch_side
    from gsn_amd.step import CountLayerStep
    dev = torch.device("cuda", 0)
    classes = list(classes)
    node_ptr, edge_ptr, ei = _collate(graphs, ids_are_global)
    N, E = int(node_ptr[-1]), int(edge_ptr[-1])
    mn = int(np.diff(node_ptr).max()) if max_nodes is None else max_nodes
    me = int(np.diff(edge_ptr).max()) if max_edges is None else max_edges
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(E)
    xc, efc = layers.Codes(t(rng.integers(0, 28, N)), [28]), layers.Codes(t(rng.integers(0, 4, E)), [4])
    want = np.concatenate(want_ids, axis=0)
    bits = _hot_bits(want, classes, clamp)
    for g in blank:
        bits[edge_ptr[g]:edge_ptr[g + 1]] = 0
    plan = CountPlan.get(CYCLES, "edge", False)

    def rows():
        if not misaligned:
            return None
        flat = torch.full((4 * E + 1,), -7, dtype=torch.int64, device=dev)
        out = flat[1:].view(E, 4)
        assert out.data_ptr() % 16 == 8
        return out

    # the key step: CycKeys
    step = CountLayerStep(plan, layer, classes, clamp=clamp)
    capfd.readouterr()
    ids, _, status = step(t(node_ptr), t(edge_ptr), t(ei), xc, efc, mn, me, ids_out=rows(), ids_are_global=ids_are_global)
    torch.cuda.synchronize()
    assert step.on_keys and "cycle walk 1" in capfd.readouterr().err
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), want)
    assert np.array_equal(step._bufs[1]["idmask"][:E].cpu().numpy().astype(np.int64) & 0xffff, bits)
    assert status.cpu().tolist() == list(want_status)
    # the row-pack launch: CycAny
    r = count_batch_side(plan, t(node_ptr), t(edge_ptr), t(ei), mn, me, id_classes=classes, clamp=clamp, out=rows(), ids_are_global=ids_are_global,
                         register=False, n_nodes=N)
    torch.cuda.synchronize()
    assert "cycle walk 1" in capfd.readouterr().err
    assert np.array_equal(r["ids"].cpu().numpy(), want)
    pack = r["edge_pack"].view(torch.int16).cpu().numpy()[:, :sum(classes)]
    hot = np.where((bits[:, None] >> np.arange(sum(classes))[None, :]) & 1, np.float16(1.0), np.float16(0.0)).astype(np.float16)
    assert np.array_equal(pack, hot.view(np.int16))
    assert r["status"].cpu().tolist() == list(want_status)


def _trip_boundary_graphs():
    """Five pairs of 63, 64, 65, 127 and 128 columns (the row loop's trips of 64), a graph without a column in a pair, and an eleventh...
    thirteenth graph: the last workgroup holds one graph."""
    graphs = []
    for seed, (ma, mb, loops) in enumerate([(15, 16, 1), (15, 17, 0), (15, 17, 1), (31, 32, 1), (32, 32, 0)]):
        graphs += [_random_graph(10 + seed, 20, ma), _random_graph(20 + seed, 20, mb, loops)]
    for i, cols in enumerate([63, 64, 65, 127, 128]):
        assert graphs[2 * i][1].shape[1] + graphs[2 * i + 1][1].shape[1] == cols
    graphs += [(7, np.zeros((2, 0), dtype=np.int64)), _ring(6, [(0, 3)]), _ring(5)]
    assert len(graphs) % 2 == 1
    return graphs


@pytest.mark.parametrize("ids_are_global", [True, False])
def test_row_loop_trip_boundaries_odd_graph_count_and_an_empty_graph(capfd, layer, ids_are_global):
    graphs = _trip_boundary_graphs()
    want = [_oracle(n, ei) for n, ei in graphs]
    assert np.concatenate(want).max() > 2 and all(w.shape[0] == ei.shape[1] for w, (_, ei) in zip(want, graphs))
    _check(capfd, layer, graphs, want, [0] * len(graphs), ids_are_global=ids_are_global)


def test_rows_that_start_8_bytes_behind_a_16_byte_boundary(capfd, layer):
    graphs = _trip_boundary_graphs()
    _check(capfd, layer, graphs, [_oracle(n, ei) for n, ei in graphs], [0] * len(graphs), misaligned=True)


def test_unclamped_classes(capfd, layer):
    """Counts beyond a column's classes set no bit (and none in the pack)."""
    graphs = _trip_boundary_graphs()
    want = [_oracle(n, ei) for n, ei in graphs]
    assert (np.concatenate(want) >= np.array([2, 3, 3, 4])).any(axis=0).all()
    _check(capfd, layer, graphs, want, [0] * len(graphs), classes=(2, 3, 3, 4), clamp=False)


def test_pair_of_33_and_32_vertices_takes_the_single_passes(capfd, layer):
    graphs = [_ring(33, [(0, 5), (2, 7), (10, 13)]), _ring(32, [(0, 4), (1, 3)])]
    want = [_oracle(n, ei) for n, ei in graphs]
    assert all(w.max() > 0 for w in want)
    _check(capfd, layer, graphs, want, [0, 0])


def test_self_loops_duplicates_and_a_one_way_column(capfd, layer):
    """The last duplicate carries the counts, superseded columns and self loops are zero rows; 3 -> 0 without 0 -> 3: KEYERROR, the rows
    that exist carry the counts of the undirected graph."""
    ring = np.concatenate([_both([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 3)]), np.array([[0, 2], [1, 2]])], axis=1)   # (0,1) again, loop at 2
    w_ring = _oracle(6, ring)
    first = int(np.flatnonzero((ring[0] == 0) & (ring[1] == 1))[0])
    assert not w_ring[first].any() and w_ring[-2].any() and not w_ring[-1].any()
    square = _both([(0, 1), (1, 2), (2, 3), (3, 0)])
    keep = ~((square[0] == 0) & (square[1] == 3))
    full = _oracle(4, square)
    assert full.any()
    _check(capfd, layer, [(6, ring), (4, square[:, keep]), (4, square)], [w_ring, full[keep], full], [0, ST_KEYERROR, 0])


def test_out_of_range_index_in_either_graph_of_a_pair(capfd, layer):
    n, ring = _ring(6, [(0, 3)])
    bad = ring.copy(); bad[1, 4] = 9
    good = _oracle(6, ring)
    zeros = np.zeros_like(good)
    _check(capfd, layer, [(6, bad), (6, ring), (6, ring)], [zeros, good, good], [ST_BAD_INDEX, 0, 0], blank=[0])
    _check(capfd, layer, [(6, ring), (6, bad)], [good, zeros], [0, ST_BAD_INDEX], blank=[1])


def test_under_declared_max_nodes(capfd, layer):
    """max_nodes = 6 with a graph of 9 vertices: TOO_LARGE and zero rows for it, its neighbour in the pair and the next pair are counted."""
    graphs = [_ring(9, [(0, 4)]), _ring(6, [(0, 3)]), _ring(5), _ring(4)]
    want = [_oracle(n, ei) for n, ei in graphs]
    want[0] = np.zeros_like(want[0])
    _check(capfd, layer, graphs, want, [ST_TOO_LARGE, 0, 0, 0], blank=[0], max_nodes=6)
