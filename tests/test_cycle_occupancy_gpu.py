"""The cycle instantiation of the counting kernel at its occupancy bound (count.hip: COUNT_CYC_WAVES; 32-bit counters, whole-row staging,
arguments read where they are used, the 2-core in a register): int64 identifiers, the identifier columns of the edge pack and the status
words against oracle.counts2ids on the CPU and its clamped one-hot -- on the smallest shapes at which those changes can go wrong."""
import ctypes
import os
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
CLASSES = [3, 3, 3, 3]
ST_KEYERROR, ST_BAD_INDEX = 1, 3
I64P = ctypes.POINTER(ctypes.c_int64)


def _both(und):
    und = np.asarray(und, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([und.T, und.T[::-1]], axis=1)


def _collate(graphs):
    """[(n, local edge_index [2, E])] -> node_ptr, edge_ptr, batch-global edge_index; nothing is cleaned."""
    node_ptr, edge_ptr, cols = [0], [0], []
    for n, ei in graphs:
        cols.append(np.asarray(ei, dtype=np.int64).reshape(2, -1) + node_ptr[-1])
        node_ptr.append(node_ptr[-1] + n); edge_ptr.append(edge_ptr[-1] + cols[-1].shape[1])
    return np.asarray(node_ptr, np.int64), np.asarray(edge_ptr, np.int64), np.ascontiguousarray(np.concatenate(cols, 1))


def _oracle(n, ei):
    from oracle import oracle
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    return oracle.counts2ids("edge", False, np.array([0, n], np.int64), np.array([0, ei.shape[1]], np.int64), ei, CYCLES, n_threads=8)


def _one_hot(ids):
    """The clamped one-hot of the identifiers as fp16 bit patterns: class min(count, 2) of three per column."""
    hot = np.zeros((ids.shape[0], 12), dtype=np.float16)
    rows = np.arange(ids.shape[0])
    for c in range(4):
        hot[rows, 3 * c + np.minimum(ids[:, c], 2)] = 1.0
    return hot.view(np.int16)


def _launch(node_ptr, edge_ptr, ei, x_codes=None, ef_codes=None, csr_row=None):
    from gsn_amd.counting import CountPlan, count_batch_side
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    r = count_batch_side(CountPlan.get(CYCLES, "edge", False), t(node_ptr), t(edge_ptr), t(ei), int(np.diff(node_ptr).max()), int(np.diff(edge_ptr).max()),
                         id_classes=CLASSES, clamp=True, x_codes=x_codes, ef_codes=ef_codes, csr_row=csr_row, register=False, n_nodes=int(node_ptr[-1]))
    torch.cuda.synchronize()
    return r["ids"].cpu().numpy(), r["edge_pack"].view(torch.int16).cpu().numpy(), r["status"].cpu().numpy(), r


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")      # (read at every launch: the library names the instantiation it takes on stderr)


def _check(capfd, graphs, want_ids, want_status, blank=(), cycle_path=True, **side):
    """One launch of the collated graphs; ``blank``: graphs whose rows are reported instead of counted (zero identifiers, no class set);
    ``cycle_path``: whether the launcher's rule sends this launch down the cycle instantiation (asserted either way)."""
    node_ptr, edge_ptr, ei = _collate(graphs)
    capfd.readouterr()
    ids, pack, status, r = _launch(node_ptr, edge_ptr, ei, **side)
    assert ("cycle walk 1" in capfd.readouterr().err) == cycle_path, "the launcher's choice of instantiation"
    want = np.concatenate(want_ids, axis=0)
    assert ids.dtype == np.int64 and np.array_equal(ids, want)
    hot = _one_hot(want)
    for g in blank:
        hot[edge_ptr[g]:edge_ptr[g + 1]] = 0
    assert np.array_equal(pack[:, :12], hot)
    assert status.tolist() == list(want_status)
    return ids, pack, r


def test_odd_graph_count_with_side_outputs(capfd):
    """(a) five ZINC-shaped graphs: the last counting workgroup holds a single graph, the one side group is incomplete."""
    from gsn_amd import layers, synth
    b = synth.zinc_shape_batch(5, seed=11)
    npt, ept = np.asarray(b.node_ptr), np.asarray(b.edge_ptr)
    local = np.asarray(b.edge_index) - np.repeat(npt[:-1], np.diff(ept))[None, :]
    graphs = [(int(npt[g + 1] - npt[g]), local[:, ept[g]:ept[g + 1]]) for g in range(5)]
    want = [_oracle(n, ei) for n, ei in graphs]
    assert np.concatenate(want).max() > 0
    dev = torch.device("cuda", 0)
    x = layers.Codes(torch.from_numpy(np.asarray(b.atom_type)).to(dev), [28])
    ef = layers.Codes(torch.from_numpy(np.asarray(b.bond_type)).to(dev), [4])
    _, pack, r = _check(capfd, graphs, want, [0] * 5, x_codes=x, ef_codes=ef, csr_row=1)
    # the side workgroup's outputs of the same launch: bond columns behind the identifiers', the node pack, the CSR's segment ends
    bond = np.zeros((pack.shape[0], 4), np.float16)
    bond[np.arange(pack.shape[0]), np.asarray(b.bond_type)] = 1.0
    assert np.array_equal(pack[:, 12:16], bond.view(np.int16))
    atom = r["node_pack"].float().cpu().numpy()
    assert np.array_equal(atom[:, :28].argmax(1), np.asarray(b.atom_type)) and (atom[:, :28].sum(1) == 1).all()
    seg = r["csr"].seg_ptr.cpu().numpy()
    assert seg[0] == 0 and seg[-1] == pack.shape[0] and np.array_equal(np.diff(seg), np.bincount(np.asarray(b.edge_index)[1], minlength=int(npt[-1])))
    assert int(r["code_status"].item()) == 0


def test_pair_beyond_64_vertices_runs_the_single_passes(capfd):
    """(b) two graphs of 40 vertices: the pair does not fit one adjacency word, passes 1 and 2 run the body on one graph each."""
    from gsn_amd import synth
    rng = np.random.default_rng(5)
    graphs = []
    for _ in range(2):
        n, ei = synth.zinc_shape_graph(rng, mean_n=40, sd_n=0.0, n_min=40, n_max=40, ring_rate=5.0)
        graphs.append((int(n), np.asarray(ei)))
    assert all(n == 40 for n, _ in graphs)
    want = [_oracle(n, ei) for n, ei in graphs]
    assert all(w.max() > 0 for w in want)
    _check(capfd, graphs, want, [0, 0])


def test_dense_graph_and_ring_with_duplicate_and_self_loop(capfd):
    """(c) a random graph of 17 vertices / 64 directed columns (the dense guard of DESIGN 3c) beside a 6-ring with a chord, a
    duplicated column and a self-loop column: the last duplicate carries the counts, rows that carry nothing are zero, all four lengths
    occur, counts beyond class 2 are clamped in the pack."""
    rng = np.random.default_rng(17)
    pairs = [(u, v) for u in range(17) for v in range(u + 1, 17)]
    und = [pairs[i] for i in rng.permutation(len(pairs))[:32]]
    dense = _both(und)
    ring = np.concatenate([_both([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 3)]), np.array([[0, 2], [1, 2]])], axis=1)   # (0,1) again, loop at 2
    assert dense.shape[1] == 64
    want = [_oracle(17, dense), _oracle(6, ring)]
    assert want[0].max() > 2 and (want[0].max(axis=0) > 0).all() and (want[1].max(axis=0) > 0).all()
    first = int(np.flatnonzero((ring[0] == 0) & (ring[1] == 1))[0])
    assert not want[1][first].any() and want[1][-2].any() and not want[1][-1].any()      # superseded column, its last duplicate, the self loop
    _check(capfd, [(17, dense), (6, ring)], want, [0, 0])


@pytest.mark.parametrize("classes,clamp", [([3, 3, 3, 3], True), ([2, 3, 2, 4], False)])
def test_encoded_rows_without_counts_take_the_class_byte_arm(capfd, classes, clamp):
    """No int64 rows (counts=False): nothing is staged as 16-bit counts, so every row leaves its four class indices as ONE word of bytes --
    clamped to the last class, or none (a zero row of floats) for a count beyond the classes.  Width 11 also takes the plain row loop."""
    from gsn_amd.counting import CountPlan, count_batch
    rng = np.random.default_rng(17)
    pairs = [(u, v) for u in range(17) for v in range(u + 1, 17)]
    dense = _both([pairs[i] for i in rng.permutation(len(pairs))[:32]])
    ring = np.concatenate([_both([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 3)]), np.array([[0, 2], [1, 2]])], axis=1)
    want = np.concatenate([_oracle(17, dense), _oracle(6, ring)], axis=0)
    assert want.max() >= max(classes)
    node_ptr, edge_ptr, ei = _collate([(17, dense), (6, ring)])
    capfd.readouterr()
    out, status, enc = count_batch(CountPlan.get(CYCLES, "edge", False), node_ptr, edge_ptr, ei, ids_are_global=True, device=torch.device("cuda", 0),
                                   encode=(classes, clamp), counts=False)
    torch.cuda.synchronize()
    assert "cycle walk 1" in capfd.readouterr().err and out is None and status.cpu().tolist() == [0, 0]
    hot = np.zeros((want.shape[0], sum(classes)), dtype=np.float32)
    rows, first = np.arange(want.shape[0]), 0
    for c, ncls in enumerate(classes):
        cls = np.minimum(want[:, c], ncls - 1) if clamp else want[:, c]
        ok = cls < ncls
        hot[rows[ok], first + cls[ok]] = 1.0
        first += ncls
    assert np.array_equal(enc.cpu().numpy(), hot)


def test_missing_reverse_column_raises_keyerror_status(capfd):
    """(d) 3 -> 0 without 0 -> 3 on a ring: the reference raises KeyError as soon as a match uses the missing direction; the rows that
    exist carry the counts of the undirected graph."""
    ring = _both([(0, 1), (1, 2), (2, 3), (3, 0)])
    keep = ~((ring[0] == 0) & (ring[1] == 3))
    one_way = ring[:, keep]
    with pytest.raises(KeyError):
        _oracle(4, one_way)
    full = _oracle(4, ring)
    assert full.any()
    _check(capfd, [(4, one_way), (4, ring)], [full[keep], full], [ST_KEYERROR, 0])


def test_out_of_range_endpoint_is_reported_and_the_neighbour_is_counted(capfd):
    """(e) vertex 9 of a 6-vertex graph: BAD_INDEX, zero rows (no class set in the pack); the other graph of the pair is counted as ever."""
    ring = _both([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3)])
    bad = ring.copy(); bad[1, 4] = 9
    good = _oracle(6, ring)
    assert good.any()
    zeros = np.zeros_like(good)
    _check(capfd, [(6, bad), (6, ring), (6, ring)], [zeros, good, good], [ST_BAD_INDEX, 0, 0], blank=[0])
    _check(capfd, [(6, ring), (6, bad)], [good, zeros], [0, ST_BAD_INDEX], blank=[1])


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libcycle_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "cycle_harness.cpp")])
    return ctypes.CDLL(so)


def _ring(n):
    return _both([(i, (i + 1) % n) for i in range(n)])


def test_complete_graphs_pin_the_counter_width(capfd, harness):
    """(f) K12: 10 * 9 * 8 * 7 six-cycles through every edge.  The largest cell is computed on the CPU by cycle_walk
    (tests/cycle_harness.cpp) and must fit 32 bits; then the kernel against the oracle.  K12 has 132 columns, and the launcher keeps
    one-wave workgroups -- the cycle path among them -- to graphs of <= 128 columns, so K12 itself is counted by the interpreter (asserted:
    the rule is part of what bounds this path's counters).  K11 (110 columns, 9 * 8 * 7 * 6) is the largest complete graph ON the path;
    a 17-ring rides along so that the declared sizes stay below 8 columns per vertex, where the interpreter's tight loop takes over."""
    ring = _ring(17)
    want_ring = _oracle(17, ring)
    for n, on_path in ((12, False), (11, True)):
        kn = _both(list(nx.complete_graph(n).edges))
        src, dst = np.ascontiguousarray(kn[0]), np.ascontiguousarray(kn[1])
        walk = np.full((kn.shape[1], 4), -1, dtype=np.int64)
        assert harness.cycle_harness_walk(6, ctypes.c_int64(n), ctypes.c_int64(kn.shape[1]), src.ctypes.data_as(I64P), dst.ctypes.data_as(I64P), 1,
                                          walk.ctypes.data_as(I64P)) == 0
        assert walk.max() == (n - 2) * (n - 3) * (n - 4) * (n - 5) and walk.max() < 2 ** 32
        want = _oracle(n, kn)
        assert np.array_equal(want, walk)
        _check(capfd, [(n, kn), (17, ring)], [want, want_ring], [0, 0], cycle_path=on_path)
