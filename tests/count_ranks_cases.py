"""Batches shared by tests/test_count_ranks_gpu.py and its child process tests/count_ranks_child.py (not a test module): the smallest
shapes at which the counting launch's set-up can go wrong -- trips of 64 columns, a 64-vertex graph, pairs that are redone graph by graph,
repeated and one-way columns, endpoints outside their graph -- as plain numpy, so that both processes build the very same arrays."""
import numpy as np

ST_KEYERROR, ST_TOO_LARGE, ST_BAD_INDEX = 1, 2, 3


def both(und):
    und = np.asarray(und, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([und.T, und.T[::-1]], axis=1)


def random_graph(seed, n, m, loops=0):
    """m undirected pairs among n vertices, both directions in shuffled column order, + `loops` self-loop columns."""
    rng = np.random.default_rng(seed)
    pairs = [(u, v) for u in range(n) for v in range(u + 1, n)]
    ei = both([pairs[i] for i in rng.permutation(len(pairs))[:m]])
    ei = ei[:, rng.permutation(ei.shape[1])]
    if loops:
        ei = np.concatenate([ei, np.tile(np.arange(loops, dtype=np.int64), (2, 1))], axis=1)
    return n, ei


def ring(n, chords=()):
    return n, both([(i, (i + 1) % n) for i in range(n)] + list(chords))


def collate(graphs, ids_are_global=True):
    node_ptr, edge_ptr, cols = [0], [0], []
    for n, ei in graphs:
        cols.append(np.asarray(ei, dtype=np.int64).reshape(2, -1) + (node_ptr[-1] if ids_are_global else 0))
        node_ptr.append(node_ptr[-1] + n); edge_ptr.append(edge_ptr[-1] + cols[-1].shape[1])
    return np.asarray(node_ptr, np.int64), np.asarray(edge_ptr, np.int64), np.ascontiguousarray(np.concatenate(cols, 1))


def size_edges():
    """Pairs of 63, 64, 65, 127, 128 and 129 columns; a vertex without a column beside a single self loop; a 64-vertex graph (its pair does
    not fit 64 vertices: both graphs are redone one by one, and the single pass writes rowstart[64]); an odd graph count."""
    graphs = []
    for seed, (ma, mb, loops) in enumerate([(15, 16, 1), (16, 16, 0), (16, 16, 1), (31, 32, 1), (32, 32, 0), (32, 32, 1)]):
        graphs += [random_graph(10 + seed, 20, ma), random_graph(20 + seed, 20, mb, loops)]
    cols = [graphs[2 * i][1].shape[1] + graphs[2 * i + 1][1].shape[1] for i in range(6)]
    assert cols == [63, 64, 65, 127, 128, 129], cols
    graphs += [(1, np.zeros((2, 0), dtype=np.int64)), (1, np.zeros((2, 1), dtype=np.int64))]
    # (at most 128 columns per graph: beyond that a launch leaves the one-wave workgroups, and with them the cycle path)
    g64 = both([(i, i + 1) for i in range(58)] + [(0, 2), (0, 3), (60, 61), (61, 62), (62, 63), (63, 60)])
    graphs += [(64, g64), ring(7, [(0, 2), (0, 3)])]
    graphs += [ring(40, [(0, 2), (3, 6)]), ring(41, [(1, 3), (1, 4)])]            # 81 vertices: one by one again
    graphs += [ring(5, [(0, 2)])]
    assert len(graphs) % 2 == 1
    return graphs


def columns():
    """The same column three times (the last one carries the counts, also when the pair is redone graph by graph), a pair present in one
    direction only (KEYERROR; the rows that exist carry the undirected graph's counts), a one-way pendant on no cycle (no error)."""
    n, r6 = ring(6, [(0, 3), (1, 3)])
    thrice = np.concatenate([np.array([[0], [1]]), r6[:, :5], np.array([[0], [1]]), r6[:, 5:], np.array([[1, 0], [0, 1]])], axis=1)
    assert ((thrice[0] == 0) & (thrice[1] == 1)).sum() == 4 and ((thrice[0] == 1) & (thrice[1] == 0)).sum() == 2
    no_rev = r6[:, ~((r6[0] == 0) & (r6[1] == 3))]
    pendant = np.concatenate([both([(0, 1), (1, 2), (2, 0)]), np.array([[2], [3]])], axis=1)
    big = ring(60, [(0, 2)])
    dup_big = np.concatenate([big[1], big[1][:, :3], big[1][:, :3]], axis=1)       # three columns three times each, in a graph that is redone alone
    return [(6, thrice), (6, no_rev), (4, pendant), (6, r6), (60, dup_big), (6, thrice), (6, r6)]


def columns_status():
    return [0, ST_KEYERROR, 0, 0, 0, 0, 0]


def bad_index():
    """An endpoint at -1, at n and at 2^32 + 1 (its low word names a vertex of the graph: only the high word gives it away), as source or as
    target, in the first and in the second graph of a pair; every such graph is reported and left zero, its neighbour is counted."""
    n, r6 = ring(6, [(0, 3)])
    out = []
    for k, (row, col, val) in enumerate([(1, 4, -1), (0, 2, 6), (1, 7, (1 << 32) + 1), (0, 0, -1), (1, 13, 6), (0, 9, (1 << 32) + 1)]):
        bad = r6.copy(); bad[row, col] = val
        out += [(6, bad), (6, r6)] if k % 2 == 0 else [(6, r6), (6, bad)]
    return out


def bad_index_status():
    return [ST_BAD_INDEX, 0, 0, ST_BAD_INDEX] * 3


def one_way():
    """Every pair in one direction only: a graph then has twice as many slots of the CSR rank as columns.  Two graphs with as many columns
    as the batch declares have more slots together than a pair's table holds (redone graph by graph); paths and a star lie on no cycle
    (no error), a one-way ring is the reference's KeyError."""
    path = np.stack([np.arange(9), np.arange(1, 10)]).astype(np.int64)
    star = np.stack([np.zeros(9, np.int64), np.arange(1, 10)]).astype(np.int64)
    ring5 = np.stack([np.arange(5), (np.arange(5) + 1) % 5]).astype(np.int64)
    n, r6 = ring(6, [(0, 3)])
    return [(10, path), (10, star), (5, ring5), (10, path[::-1].copy()), (6, r6), (10, star[::-1].copy()), (10, path)]


def one_way_status():
    return [0, 0, ST_KEYERROR, 0, 0, 0, 0]


COUNT_CASES = {
    "one_way": (one_way, True, None),
    "one_way_local": (one_way, False, None),
    # name: (graphs, ids_are_global, max_nodes or None)
    "size_edges": (size_edges, True, None),
    "size_edges_local": (size_edges, False, None),
    "columns": (columns, True, None),
    "columns_local": (columns, False, None),
    "bad_index": (bad_index, True, None),
    "bad_index_local": (bad_index, False, None),
}


def count_case(name):
    """node_ptr, edge_ptr, edge_index, ids_are_global, max_nodes, max_edges of a named case; "zinc": the 2 000-graph seeded molecule batch."""
    if name == "zinc":
        from gsn_amd import synth
        b = synth.zinc_shape_batch(2000, seed=11)
        return b.node_ptr, b.edge_ptr, b.edge_index, True, int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    make, glob, mn = COUNT_CASES[name]
    node_ptr, edge_ptr, ei = collate(make(), glob)
    return node_ptr, edge_ptr, ei, glob, int(np.diff(node_ptr).max()) if mn is None else mn, int(np.diff(edge_ptr).max())


ALL_CASES = list(COUNT_CASES) + ["zinc"]
