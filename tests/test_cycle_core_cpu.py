"""CPU checks of the cycle columns' fast path (gsn_amd/csrc/count_core.h: cycle_walk, cycle_plan_lengths), compiled for the host by
the test-only harness tests/cycle_harness.cpp: the bitset path walk against the oracle, and the launcher's recognition rule on plan
tables from gsn_count_plan_build."""
import ctypes
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P, U32P, U8P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libcycle_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "cycle_harness.cpp")])
    return ctypes.CDLL(so)


def _cycles(lo, hi):
    return [list(nx.cycle_graph(k).edges) for k in range(lo, hi + 1)]


def _walk(harness, L, n, ei, prune=1):
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    E = ei.shape[1]
    src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    out = np.full((E, L - 2), -1, dtype=np.int64)
    st = harness.cycle_harness_walk(L, ctypes.c_int64(n), ctypes.c_int64(E), src.ctypes.data_as(I64P), dst.ctypes.data_as(I64P), prune,
                                    out.ctypes.data_as(I64P))
    assert st >= 0
    return out, st


def _oracle(L, n, ei):
    from oracle import oracle
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    return oracle.counts2ids("edge", False, np.array([0, n], dtype=np.int64), np.array([0, ei.shape[1]], dtype=np.int64), ei, _cycles(3, L), n_threads=4)


def _both_ways(und):
    und = np.asarray(und, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([und.T, und.T[::-1]], axis=1)


@pytest.mark.parametrize("L", [6, 8])
def test_walk_matches_oracle_on_zinc_shaped_batch(harness, L):
    """Every row of synth.zinc_shape_batch(2000, seed=7): the walk's counts for k = 3 .. L equal the oracle's identifiers of cycle_graph(k),
    edge mode, non-induced -- with the 2-core pruning the kernel uses and without it."""
    from gsn_amd import synth
    from oracle import oracle
    b = synth.zinc_shape_batch(2000, seed=7)
    npt, ept = np.asarray(b.node_ptr), np.asarray(b.edge_ptr)
    ei = np.asarray(b.edge_index)
    local = ei - np.repeat(npt[:-1], np.diff(ept))[None, :]
    ref = oracle.counts2ids("edge", False, npt, ept, local, _cycles(3, L), n_threads=8)
    assert ref.shape == (ei.shape[1], L - 2) and (ref.max(axis=0) > 0).all()
    for prune in (1, 0):
        got = np.concatenate([_walk(harness, L, int(npt[g + 1] - npt[g]), local[:, ept[g]:ept[g + 1]], prune)[0] for g in range(len(npt) - 1)], axis=0)
        assert np.array_equal(got, ref), (L, prune)


HAND_MADE = {
    "K5": (5, _both_ways(list(nx.complete_graph(5).edges))),
    "two triangles sharing an edge": (4, _both_ways([(0, 1), (1, 2), (2, 0), (1, 3), (3, 2)])),
    "6-ring with a chord": (6, _both_ways([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3)])),
    "K4 with a tail": (7, _both_ways([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 4), (4, 5), (5, 6)])),
    "8-ring fused to a 5-ring": (11, _both_ways([(i, (i + 1) % 8) for i in range(8)] + [(0, 8), (8, 9), (9, 10), (10, 1)])),
}


@pytest.mark.parametrize("L", [6, 8])
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_walk_matches_oracle_on_hand_made_graphs(harness, L, name):
    n, ei = HAND_MADE[name]
    for prune in (1, 0):
        got, st = _walk(harness, L, n, ei, prune)
        assert st == 0
        assert np.array_equal(got, _oracle(L, n, ei)), (name, L, prune)
    if name == "K5":        # paths of k - 1 edges from v to u through the other three vertices: 3, 3 * 2, 3 * 2 * 1
        assert got[0].tolist()[:3] == [3, 6, 6] and not got[:, 3:].any()


@pytest.mark.parametrize("L", [6, 8])
def test_walk_on_self_loops_and_duplicated_columns(harness, L):
    """Self-loop columns carry nothing and add no edge; of duplicated columns only the last carries the pair's counts (the reference's
    dictionary of columns keeps the last index).  The oracle restates both."""
    und = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 0)]
    ei = _both_ways(und)
    ei = np.concatenate([ei, np.array([[1, 3, 0, 2], [1, 3, 1, 0]])], axis=1)      # two self loops, (0,1) and (2,0) a second time
    got, st = _walk(harness, L, 5, ei)
    assert st == 0
    ref = _oracle(L, 5, ei)
    assert np.array_equal(got, ref)
    assert not got[0].any() and got[-2].any() and not got[-4].any() and not got[-3].any()      # first (0,1): superseded; self loops: zero


@pytest.mark.parametrize("L", [6, 8])
def test_walk_with_a_missing_reverse_column(harness, L):
    """A pair present in one direction only: the reference raises KeyError as soon as a match uses the missing direction -- status 1 here,
    KeyError from the oracle; a one-way pendant edge lies on no cycle and raises nothing."""
    ring = _both_ways([(0, 1), (1, 2), (2, 3), (3, 0)])
    pendant = np.concatenate([ring, np.array([[3], [4]])], axis=1)
    got, st = _walk(harness, L, 5, pendant)
    assert st == 0 and np.array_equal(got, _oracle(L, 5, pendant)) and not got[-1].any() and got[0, 1] == 1
    one_way = ring[:, ~((ring[0] == 0) & (ring[1] == 3))]                          # 3 -> 0 without 0 -> 3
    got, st = _walk(harness, L, 4, one_way)
    assert st == 1
    with pytest.raises(KeyError):
        _oracle(L, 4, one_way)


def _recognise(harness, plan, cap=8):
    table = np.ascontiguousarray(plan.table)
    length = np.zeros(cap, dtype=np.uint8)
    lmax = harness.cycle_harness_recognise(table.ctypes.data_as(U32P), ctypes.c_int64(len(table)), length.ctypes.data_as(U8P), cap)
    return lmax, length[:plan.n_cols].tolist()


class _Table:
    def __init__(self, table, n_cols):
        self.table, self.n_cols = table, n_cols


def _two_triangles_table(plan):
    """The 6-cycle's table with its level masks rewritten to two disjoint triangles {0, 1, 2}, {3, 4, 5}: six vertices, six edges, every
    degree 2 -- and not one cycle."""
    t = plan.table.copy()
    off = int(t[7])
    assert int(t[off]) & 0xff == 6
    for l, adj in enumerate([0, 0b1, 0b11, 0, 0b1000, 0b11000]):
        t[off + 2 + l] = adj
    return _Table(t, plan.n_cols)


def test_recognition_accepts_cycle_plans(lib, harness):
    from gsn_amd.counting import CountPlan
    assert _recognise(harness, CountPlan(_cycles(3, 8), "edge", False)) == (8, [3, 4, 5, 6, 7, 8])
    assert _recognise(harness, CountPlan(_cycles(3, 6), "edge", False)) == (6, [3, 4, 5, 6])
    assert _recognise(harness, CountPlan([_cycles(3, 6)[i] for i in (2, 0, 3, 1)], "edge", False)) == (6, [5, 3, 6, 4])
    # a relabelled cycle is a cycle: recognition reads the plan's structure, not a name
    assert _recognise(harness, CountPlan([[(0, 3), (3, 1), (1, 4), (4, 2), (2, 0)]], "edge", False)) == (5, [5])
    assert _recognise(harness, CountPlan(_cycles(3, 6), "edge", False), cap=3)[0] == 0       # more columns than the caller takes


@pytest.mark.parametrize("what", ["induced", "vertex", "directed orbits", "cliques", "path", "cycle + clique", "two cycles", "theta"])
def test_recognition_refuses_everything_else(lib, harness, what):
    from gsn_amd.counting import CountPlan
    cliques = [list(nx.complete_graph(k).edges) for k in (3, 4, 5)]
    plan = {
        "induced": lambda: CountPlan(_cycles(3, 8), "edge", True),
        "vertex": lambda: CountPlan(_cycles(3, 8), "vertex", False),
        "directed orbits": lambda: CountPlan(_cycles(3, 8), "edge", False, True),
        "cliques": lambda: CountPlan(cliques, "edge", False),
        "path": lambda: CountPlan([list(nx.path_graph(4).edges)], "edge", False),
        "cycle + clique": lambda: CountPlan(_cycles(3, 5) + [cliques[1]], "edge", False),
        "two cycles": lambda: _two_triangles_table(CountPlan(_cycles(6, 6), "edge", False)),
        "theta": lambda: CountPlan([[(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]], "edge", False),
    }[what]()
    assert _recognise(harness, plan, cap=64)[0] == 0
    if what == "induced":       # each induced cycle alone as well (the induced triangle has no non-edge to forbid: the header says induced)
        for k in range(3, 9):
            assert _recognise(harness, CountPlan(_cycles(k, k), "edge", True))[0] == 0
    if what == "vertex":        # directed plans are vertex-mode plans
        assert _recognise(harness, CountPlan([[(0, 1), (1, 2), (2, 0)]], "vertex", False, False, directed=True), cap=64)[0] == 0
