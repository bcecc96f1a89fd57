"""CPU checks of the sparse counting kernel's search core (gsn_amd/csrc/count_sparse_core.h), compiled for the host by the test-only
harness tests/sparse_harness.cpp: plans from gsn_count_plan_build, searched over sorted neighbour lists, against the oracle."""
import ctypes
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P, U32P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)
SRC = os.path.join(REPO, "tests", "sparse_harness.cpp")


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libsparse_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def _families():
    from networkx.generators.atlas import graph_atlas_g
    five = [list(g.edges) for g in graph_atlas_g() if g.number_of_nodes() == 5 and nx.is_connected(g)]
    assert len(five) == 21
    return {
        "cycles": [list(nx.cycle_graph(k).edges) for k in range(3, 7)],
        "cliques": [list(nx.complete_graph(k).edges) for k in range(3, 6)],
        "paths": [list(nx.path_graph(k).edges) for k in range(3, 7)],
        "stars": [list(nx.star_graph(k - 1).edges) for k in range(3, 6)],
        "five": five,
    }


def _count(harness, plan, n, ei):
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    E = ei.shape[1]
    src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    rows = E if plan.mode == "edge" else n
    out = np.full((rows, plan.n_cols), -1, dtype=np.int64)
    st = harness.sparse_harness_count(plan.table.ctypes.data_as(U32P), ctypes.c_int64(n), ctypes.c_int64(E), src.ctypes.data_as(I64P),
                                      dst.ctypes.data_as(I64P), out.ctypes.data_as(I64P))
    return out, st


def _oracle(mode, induced, n, ei, pats):
    from oracle import oracle
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    return oracle.counts2ids(mode, induced, np.array([0, n], dtype=np.int64), np.array([0, ei.shape[1]], dtype=np.int64), ei, pats, n_threads=8)


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
@pytest.mark.parametrize("family", ["cycles", "cliques", "paths", "stars", "five"])
def test_core_matches_oracle_on_small_random_graphs(lib, harness, family, mode, induced):
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    pats = _families()[family]
    plan = CountPlan(pats, mode, induced)
    for n, ei in (synth.er_graph(11, 22, 3), synth.er_graph(14, 30, 1)):
        got, st = _count(harness, plan, n, ei)
        ref = _oracle(mode, induced, n, ei, pats)
        assert st == 0 and got.shape == ref.shape
        assert np.array_equal(got, ref)
        assert ref.sum() > 0


@pytest.fixture(scope="module")
def zinc769():
    from gsn_amd import synth
    n, ei = synth.zinc_shape_graph(np.random.default_rng(769), mean_n=769, sd_n=0.0, n_min=769, n_max=769, ring_rate=40.0)
    assert n == 769
    return n, ei


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
def test_core_matches_oracle_on_769_vertices(lib, harness, zinc769, mode, induced):
    """One vertex more than the LDS kernel takes: cycles 3-6 and cliques 3-5."""
    from gsn_amd.counting import CountPlan
    n, ei = zinc769
    fam = _families()
    pats = fam["cycles"] + fam["cliques"]
    got, st = _count(harness, CountPlan(pats, mode, induced), n, ei)
    ref = _oracle(mode, induced, n, ei, pats)
    assert st == 0 and np.array_equal(got, ref)
    assert ref.sum() > 0


def test_duplicate_column_and_self_loop(lib, harness):
    """The last duplicate of a column holds the counts; earlier duplicates and self loops are zero rows (utils_graph_processing.py:142-144).
    Vertex counts do not see either."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    n, ei = synth.er_graph(11, 22, 3)
    E = ei.shape[1]
    pats = _families()["cycles"]
    ref = _oracle("edge", False, n, ei, pats)
    c = int(np.nonzero(ref.sum(1))[0][0])
    ei2 = np.concatenate([ei, ei[:, c:c + 1], np.array([[2], [2]])], axis=1)
    got, st = _count(harness, CountPlan(pats, "edge", False), n, ei2)
    want = np.concatenate([ref, ref[c:c + 1], np.zeros((1, ref.shape[1]), np.int64)], axis=0)
    want[c] = 0
    assert st == 0 and np.array_equal(got, want) and want[E].sum() > 0
    got_v, st_v = _count(harness, CountPlan(pats, "vertex", False), n, ei2)
    assert st_v == 0 and np.array_equal(got_v, _oracle("vertex", False, n, ei, pats))


def test_missing_reverse_column_is_a_keyerror(lib, harness):
    """A column on a triangle whose reverse is no column: the reference raises KeyError (utils_graph_processing.py:173)."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    n, ei = synth.er_graph(11, 22, 3)
    pats = [list(nx.cycle_graph(3).edges)]
    ref = _oracle("edge", False, n, ei, pats)
    c = int(np.nonzero(ref[:, 0])[0][0])
    rev = int(np.nonzero((ei[0] == ei[1, c]) & (ei[1] == ei[0, c]))[0][0])
    got, st = _count(harness, CountPlan(pats, "edge", False), n, np.delete(ei, rev, axis=1))
    assert st == 1
    # a column that no triangle touches may lose its reverse
    c0 = int(np.nonzero(ref[:, 0] == 0)[0][0])
    rev0 = int(np.nonzero((ei[0] == ei[1, c0]) & (ei[1] == ei[0, c0]))[0][0])
    got, st = _count(harness, CountPlan(pats, "edge", False), n, np.delete(ei, rev0, axis=1))
    assert st == 0 and np.array_equal(got, np.delete(ref, rev0, axis=0))
    # an endpoint outside the graph
    bad = ei.copy()
    bad[1, 3] = n
    assert _count(harness, CountPlan(pats, "edge", False), n, bad)[1] == 3


def test_harness_under_address_and_undefined_sanitizers(lib, zinc769):
    """The same core as a stand-alone program built with -fsanitize=address,undefined, on one small case with a duplicated column and a self
    loop and on the 769-vertex graph."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    exe = os.path.join(REPO, "tests", "_build", "sparse_harness_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSPARSE_HARNESS_MAIN", "-o", exe, SRC])
    fam = _families()
    n, ei = synth.er_graph(11, 22, 3)
    ei = np.concatenate([ei, ei[:, :1], np.array([[2], [2]])], axis=1)
    cases = [("small", fam["five"] + fam["stars"] + fam["paths"], "edge", True, n, ei), ("n769", fam["cycles"] + fam["cliques"], "vertex", False) + zinc769]
    for name, pats, mode, induced, n, ei in cases:
        plan = CountPlan(pats, mode, induced)
        ei = np.ascontiguousarray(ei, dtype=np.int64)
        # expected: the oracle on the columns without the two appended ones, rearranged as test_duplicate_column_and_self_loop does
        if name == "small":
            ref = _oracle(mode, induced, n, ei[:, :-2], pats)
            want = np.concatenate([ref, ref[:1], np.zeros((1, ref.shape[1]), np.int64)], axis=0)
            want[0] = 0
        else:
            want = _oracle(mode, induced, n, ei, pats)
        path = os.path.join(REPO, "tests", "_build", "sparse_case_%s.bin" % name)
        table = plan.table if len(plan.table) % 2 == 0 else np.concatenate([plan.table, np.zeros(1, np.uint32)])
        with open(path, "wb") as f:
            f.write(np.array([len(plan.table), n, ei.shape[1], plan.n_cols, 0], dtype=np.int64).tobytes())
            f.write(table.astype(np.uint32).tobytes())
            f.write(np.ascontiguousarray(ei[0]).tobytes() + np.ascontiguousarray(ei[1]).tobytes())
            f.write(np.ascontiguousarray(want, dtype=np.int64).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("sparse harness ok:")
