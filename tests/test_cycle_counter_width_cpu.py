"""Counter width of the cycle walk (gsn_amd/csrc/count_core.h: CycleAcc, cycle_walk), on the host through tests/cycle_harness.cpp.

The kernel's cycle instantiation (L = 6) keeps 32-bit counters from the walk to the int64 store.  The launcher takes that path for any
one-word graph (<= 64 vertices) without a condition on density, so 32 bits must hold every count such a graph can produce.  A cell for
length k counts simple paths of k - 1 edges between the row's endpoints, i.e. ordered choices of k - 2 inner vertices among the n - 2
others: at most (n - 2)! / (n - k)!, reached by the complete graph, and adding an edge never lowers a non-induced count -- K64 is the
worst case: 62 * 61 * 60 * 59 = 13 388 280 < 2^32 for k = 6.  (k = 8 on K64 is 4.4e10: cycle_walk<8> keeps 64-bit counters.)  The launcher
is stricter than that still -- one-wave workgroups take graphs of <= 128 columns, K11 at the most (tests/test_cycle_occupancy_gpu.py) --
but the width does not lean on it."""
import ctypes
import math
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libcycle_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "cycle_harness.cpp")])
    return ctypes.CDLL(so)


def _walk(harness, L, n, ei):
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    out = np.full((ei.shape[1], L - 2), -1, dtype=np.int64)
    st = harness.cycle_harness_walk(L, ctypes.c_int64(n), ctypes.c_int64(ei.shape[1]), src.ctypes.data_as(I64P), dst.ctypes.data_as(I64P), 1,
                                    out.ctypes.data_as(I64P))
    assert st >= 0
    return out


def _complete_cell(n, k):
    """k-cycles through one edge of K_n: ordered choices of the k - 2 inner vertices (exact Python integers)."""
    return math.factorial(n - 2) // math.factorial(n - k)


def test_k16_32_bit_counters_equal_64_bit_counters(harness):
    """cycle_walk<6> (32-bit counters) against cycle_walk<8> (64-bit counters) on every row of K16, and both against the closed form."""
    und = np.asarray(list(nx.complete_graph(16).edges), dtype=np.int64)
    ei = np.concatenate([und.T, und.T[::-1]], axis=1)
    narrow, wide = _walk(harness, 6, 16, ei), _walk(harness, 8, 16, ei)
    assert np.array_equal(narrow, wide[:, :4])
    assert (narrow == np.array([_complete_cell(16, k) for k in (3, 4, 5, 6)])).all()
    assert (wide[:, 4:] == np.array([_complete_cell(16, 7), _complete_cell(16, 8)])).all() and wide.max() < 2 ** 32


def test_k64_the_densest_one_word_graph_fits_32_bits(harness):
    """The largest counts the launcher can send down the path: K64.  The walk's 32-bit counters give the exact closed form (64-bit and
    wider arithmetic on the Python side), so no launch condition on density is needed; the bound for L = 8 shows why that walk is 64-bit.
    (One column per undirected pair: the harness builds both directions of the adjacency from it and walks 2 016 rows instead of 4 032.)"""
    und = np.asarray(list(nx.complete_graph(64).edges), dtype=np.int64)
    got = _walk(harness, 6, 64, und.T)
    want = [_complete_cell(64, k) for k in (3, 4, 5, 6)]
    assert want == [62, 62 * 61, 62 * 61 * 60, 62 * 61 * 60 * 59] and max(want) < 2 ** 32
    assert (got == np.array(want)).all()
    assert _complete_cell(64, 8) >= 2 ** 32
