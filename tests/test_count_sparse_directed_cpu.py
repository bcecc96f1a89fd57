"""CPU checks of the sparse counting kernel's search core (gsn_amd/csrc/count_sparse_core.h) on DIRECTED plans, compiled for the host by the
test-only harness tests/sparse_directed_harness.cpp: plans from gsn_count_plan_build with the directed flag, searched over sorted out- and
in-lists, against the reference's goldens (counts_directed.npz), the oracle and the undirected instantiation of the same core."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import case_names, count_case, directed_patterns

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P, U32P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)
SRC = os.path.join(REPO, "tests", "sparse_directed_harness.cpp")

CYCLE6 = [(i, (i + 1) % 6) for i in range(6)]
SIX = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5)]
UND = [[(0, 1), (1, 2), (2, 0)], [(i, (i + 1) % 6) for i in range(6)], [(0, 1), (0, 2), (0, 3)], [(0, 1), (1, 2), (2, 3)]]
BOTH = [el + [(v, u) for u, v in el] for el in UND]


def _patterns():
    return [el for el, _, _ in directed_patterns()] + [CYCLE6, SIX]


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libsparse_directed_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def _count(harness, plan, n, ei):
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    out = np.full((n, plan.n_cols), -1, dtype=np.int64)
    st = harness.sparse_directed_harness_count(plan.table.ctypes.data_as(U32P), ctypes.c_int64(n), ctypes.c_int64(ei.shape[1]),
                                               src.ctypes.data_as(I64P), dst.ctypes.data_as(I64P), out.ctypes.data_as(I64P))
    return out, st


def _oracle(induced, n, ei, pats):
    from oracle import oracle
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    return oracle.counts2ids("vertex", induced, np.array([0, n], dtype=np.int64), np.array([0, ei.shape[1]], dtype=np.int64), ei, pats,
                             n_threads=8, directed=True)


def _digraph(seed, n, m, dups, loops, anti):
    """m random arcs without self loops, then `dups` repeated arcs, `anti` reversed ones and `loops` self loops, shuffled."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=m)
    dst = (src + rng.integers(1, n, size=m)) % n
    ei = np.stack([src, dst]).astype(np.int64)
    lv = rng.integers(0, n, size=loops)
    ei = np.concatenate([ei, ei[:, :dups], ei[::-1, dups:dups + anti], np.stack([lv, lv])], axis=1)
    return n, np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


@pytest.mark.parametrize("name", case_names("counts_directed"))
def test_core_matches_the_reference_goldens(lib, harness, name):
    from gsn_amd.counting import CountPlan
    c = count_case(name, "counts_directed")
    plan = CountPlan(c["patterns"], "vertex", c["induced"], False, directed=True)
    npt, ept = c["node_ptr"], c["edge_ptr"]
    assert c["counts"].sum() > 0
    for g in range(len(npt) - 1):
        got, st = _count(harness, plan, int(npt[g + 1] - npt[g]), c["edge_index_local"][:, ept[g]:ept[g + 1]])
        assert st == 0 and np.array_equal(got, c["counts"][npt[g]:npt[g + 1]])


@pytest.mark.parametrize("induced", [False, True])
def test_core_matches_oracle_on_small_random_digraphs(lib, harness, induced):
    """11 and 14 vertices, 2-3 arcs per vertex, with repeated arcs, self loops and antiparallel pairs."""
    from gsn_amd.counting import CountPlan
    pats = _patterns()
    plan = CountPlan(pats, "vertex", induced, False, directed=True)
    for n, ei in (_digraph(3, 11, 26, 3, 2, 4), _digraph(1, 14, 36, 4, 3, 6)):
        got, st = _count(harness, plan, n, ei)
        ref = _oracle(induced, n, ei, pats)
        assert st == 0 and got.shape == ref.shape
        assert ref.sum() > 0
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("induced", [False, True])
def test_core_matches_oracle_on_769_vertices(lib, harness, induced):
    """One vertex more than the LDS kernel takes, 3 000 random arcs."""
    from gsn_amd.counting import CountPlan
    pats = _patterns()
    n, ei = _digraph(769, 769, 3000, 0, 0, 0)
    got, st = _count(harness, CountPlan(pats, "vertex", induced, False, directed=True), n, ei)
    ref = _oracle(induced, n, ei, pats)
    assert ref.sum() > 0
    assert st == 0 and np.array_equal(got, ref)


@pytest.mark.parametrize("induced", [False, True])
def test_symmetric_digraph_equals_undirected_core(lib, harness, induced):
    """Both arcs of every edge, bidirected patterns: the undirected patterns' counts from the undirected instantiation of the same core."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    zn, zei = synth.zinc_shape_graph(np.random.default_rng(769), mean_n=769, sd_n=0.0, n_min=769, n_max=769, ring_rate=40.0)
    assert zn == 769
    for n, ei in (synth.er_graph(14, 30, 1), (zn, zei)):
        ei = np.asarray(ei)
        pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
        assert all((v, u) in pairs for u, v in pairs)                  # (the edge lists hold both arcs of every edge)
        und, st_u = _count(harness, CountPlan(UND, "vertex", induced), n, ei)
        got, st = _count(harness, CountPlan(BOTH, "vertex", induced, False, directed=True), n, ei)
        assert st == 0 and st_u == 0
        assert und.sum() > 0
        assert np.array_equal(got, und)


def test_bad_endpoint_and_edge_plans(lib, harness):
    from gsn_amd.counting import CountPlan
    n, ei = _digraph(3, 11, 26, 0, 0, 0)
    plan = CountPlan([[(0, 1), (1, 2), (2, 0)]], "vertex", False, False, directed=True)
    bad = ei.copy()
    bad[1, 3] = n
    assert _count(harness, plan, n, bad)[1] == 3
    assert _count(harness, CountPlan(UND, "edge", False), n, ei)[1] == -1       # (the harness runs vertex plans; directed edge plans do not exist)
    with pytest.raises(Exception):
        CountPlan(BOTH, "edge", False, False, directed=True)


def test_harness_under_address_and_undefined_sanitizers():
    """The same core as a stand-alone program built with -fsanitize=address,undefined and linked with the plan compiler: a seeded digraph with
    repeated arcs, self loops and antiparallel pairs, and a bidirected graph against the undirected instantiation, induced and not."""
    exe = os.path.join(REPO, "tests", "_build", "sparse_directed_harness_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSPARSE_HARNESS_MAIN", "-o", exe, SRC, os.path.join(REPO, "gsn_amd", "csrc", "patterns.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("sparse directed harness ok:")
