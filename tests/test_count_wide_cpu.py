"""CPU checks of WIDE counting plans: pattern lists whose largest pattern has 10 .. 16 vertices (gsn_count_plan_build with GSN_FLAG_WIDE,
``CountPlan(..., wide=True)``).  The wide instantiation of the sparse kernel's search core (gsn_amd/csrc/count_sparse_core.h) is compiled for
the host by the test-only harness tests/sparse_wide_harness.cpp; the oracle (patterns of up to 16 vertices) is the referee, cell by cell."""
import ctypes
import hashlib
import json
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P, U32P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)
SRC = os.path.join(REPO, "tests", "sparse_wide_harness.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "plan_tables_narrow.json")


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libsparse_wide_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, SRC])
    return ctypes.CDLL(so)


def _el(g):
    return [(int(u), int(v)) for u, v in nx.convert_node_labels_to_integers(g).edges]


def pattern_lists():
    """name -> pattern edge lists; every list has a pattern of more than nine vertices"""
    return {
        "cycles10_16": [_el(nx.cycle_graph(k)) for k in range(10, 17)],
        "paths": [_el(nx.path_graph(k)) for k in (10, 12, 16)],
        "binomial4": [_el(nx.binomial_tree(4))],
        "trees10": [_el(t) for t in list(nx.nonisomorphic_trees(10))[:12]],
        "star9": [_el(nx.star_graph(9))],
        "petersen": [_el(nx.petersen_graph())],
        "k55": [_el(nx.complete_bipartite_graph(5, 5))],
        "mixed3_12": [_el(nx.cycle_graph(k)) for k in range(3, 13)],
    }


def _graph(g):
    g = nx.convert_node_labels_to_integers(g)
    e = np.array(list(g.edges), dtype=np.int64).reshape(-1, 2).T
    return g.number_of_nodes(), np.ascontiguousarray(np.concatenate([e, e[::-1]], axis=1))


def targets():
    from gsn_amd import synth
    pet = nx.petersen_graph()
    pet.add_edge(0, 10)
    return {
        "hypercube4": _graph(nx.hypercube_graph(4)),
        "ladder8": _graph(nx.ladder_graph(8)),
        "grid3x6": _graph(nx.grid_2d_graph(3, 6)),
        "circular_ladder9": _graph(nx.circular_ladder_graph(9)),
        "petersen_pendant": _graph(pet),
        "er14": synth.er_graph(14, 30, 1),
    }


def _count(harness, plan, n, ei):
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    E = ei.shape[1]
    src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    rows = E if plan.mode == "edge" else n
    out = np.full((rows, plan.n_cols), -1, dtype=np.int64)
    st = harness.sparse_wide_harness_count(plan.table.ctypes.data_as(U32P), ctypes.c_int64(n), ctypes.c_int64(E), src.ctypes.data_as(I64P),
                                           dst.ctypes.data_as(I64P), out.ctypes.data_as(I64P))
    return out, st


def _oracle(mode, induced, n, ei, pats, directed=False):
    from oracle import oracle
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    return oracle.counts2ids(mode, induced, np.array([0, n], dtype=np.int64), np.array([0, ei.shape[1]], dtype=np.int64), ei, pats, n_threads=8,
                             directed=directed)


# (target, pattern list, induced) -> the cycle lengths whose column the oracle must find non-zero; cycles have one orbit, so in the list
# "cycles10_16" the column of length k is k - 10
_NONZERO_CYCLES = {("hypercube4", False): (10, 12, 14, 16), ("grid3x6", True): (10, 12, 14), ("circular_ladder9", False): (11, 13, 15)}


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
@pytest.mark.parametrize("target", ["hypercube4", "ladder8", "grid3x6", "circular_ladder9", "petersen_pendant", "er14"])
def test_wide_plans_match_oracle(lib, harness, target, mode, induced):
    from gsn_amd.counting import CountPlan
    n, ei = targets()[target]
    total = 0
    for name, pats in pattern_lists().items():
        plan = CountPlan(pats, mode, induced, wide=True)
        assert plan.wide and plan.kmax > 9
        got, st = _count(harness, plan, n, ei)
        ref = _oracle(mode, induced, n, ei, pats)
        assert st == 0 and got.shape == ref.shape, name
        assert np.array_equal(got, ref), name
        total += int(ref.sum())
        if name == "cycles10_16":
            for k in _NONZERO_CYCLES.get((target, induced), ()):
                assert ref[:, k - 10].sum() > 0, (target, k)
    assert total > 0


def test_hypercube_cycle_sums(lib, harness):
    """Non-induced even cycles of the 4-cube, vertex mode: the column sums (k times the number of k-cycles)."""
    from gsn_amd.counting import CountPlan
    n, ei = targets()["hypercube4"]
    pats = pattern_lists()["cycles10_16"]
    got, st = _count(harness, CountPlan(pats, "vertex", False, wide=True), n, ei)
    assert st == 0 and got.sum(0)[[0, 2, 4, 6]].tolist() == [21120, 60288, 75264, 21504]


@pytest.fixture(scope="module")
def zinc769():
    from gsn_amd import synth
    n, ei = synth.zinc_shape_graph(np.random.default_rng(769), mean_n=769, sd_n=0.0, n_min=769, n_max=769, ring_rate=40.0)
    assert n == 769
    return n, ei


def zinc769_patterns():
    return [_el(nx.cycle_graph(10)), _el(nx.cycle_graph(12)), _el(nx.path_graph(10))]


@pytest.mark.parametrize("induced", [False, True])
@pytest.mark.parametrize("mode", ["vertex", "edge"])
def test_wide_plans_on_769_vertices(lib, harness, zinc769, mode, induced):
    from gsn_amd.counting import CountPlan
    n, ei = zinc769
    pats = zinc769_patterns()
    got, st = _count(harness, CountPlan(pats, mode, induced, wide=True), n, ei)
    ref = _oracle(mode, induced, n, ei, pats)
    assert st == 0 and np.array_equal(got, ref)
    assert ref.sum() > 0


def directed_cases():
    """(patterns, n, edge_index) of the directed wide cases: a directed 10-cycle and a directed 12-path as patterns; a digraph with both planted
    under random arcs (non-induced matches) and one that holds them as induced subgraphs."""
    pats = [[(i, (i + 1) % 10) for i in range(10)], [(i, i + 1) for i in range(11)]]
    rng = np.random.default_rng(5)
    n1 = 15
    arcs = [(i, i + 1) for i in range(n1 - 1)] + [(9, 0)]
    arcs += [(int(a), int(b)) for a, b in rng.integers(0, n1, size=(9, 2)) if a != b]
    g1 = np.ascontiguousarray(np.array(arcs, dtype=np.int64).T)
    # a directed 10-cycle with a tail in and a tail out, and a separate directed path of 13 vertices
    arcs2 = [(i, (i + 1) % 10) for i in range(10)] + [(10, 0), (5, 11)] + [(12 + i, 13 + i) for i in range(12)]
    g2 = np.ascontiguousarray(np.array(arcs2, dtype=np.int64).T)
    return pats, [(n1, g1), (25, g2)]


@pytest.mark.parametrize("induced", [False, True])
def test_directed_wide_plans_match_oracle(lib, harness, induced):
    from gsn_amd.counting import CountPlan
    pats, graphs = directed_cases()
    plan = CountPlan(pats, "vertex", induced, False, directed=True, wide=True)
    assert plan.wide
    refs = []
    for n, ei in graphs:
        got, st = _count(harness, plan, n, ei)
        refs.append(_oracle("vertex", induced, n, ei, pats, directed=True))
        assert st == 0 and np.array_equal(got, refs[-1])
    assert (refs[1].sum(0) > 0).all()               # (the second digraph holds both patterns as induced subgraphs)
    if not induced:
        assert (refs[0].sum(0) > 0).all()


@pytest.mark.parametrize("name", list(pattern_lists()))
def test_orbits_match_oracle(lib, name):
    import contextlib, io
    from gsn_amd import patterns
    from oracle import oracle
    for el in pattern_lists()[name]:
        _, part, memb, aut = patterns.automorphism_orbits(edge_list=el, print_msgs=False)
        o_memb, o_n, o_aut = oracle.automorphism_orbits(el)
        assert [memb[v] for v in range(len(memb))] == o_memb.tolist() and len(part) == o_n and aut == o_aut
        for dirorb in (False, True):
            with contextlib.redirect_stdout(io.StringIO()):
                _, epart, ememb, eaut = patterns.induced_edge_automorphism_orbits(edge_list=el, directed_orbits=dirorb)
            arcs, o_em, o_en, o_eaut = oracle.induced_edge_orbits(el, dirorb)
            assert [ememb[i] for i in range(len(ememb))] == o_em.tolist() and len(epart) == o_en and eaut == o_eaut
            assert sorted(a for v in epart.values() for a in v) == [tuple(a) for a in arcs.tolist()]


def test_refusals(lib):
    from gsn_amd import _abi
    from gsn_amd.counting import CountPlan
    c10 = _el(nx.cycle_graph(10))
    with pytest.raises(_abi.GsnError, match="k <= 9"):
        CountPlan([c10], "vertex", False)
    plan = CountPlan([c10], "vertex", False, wide=True)
    assert plan.wide and plan.kmax == 10
    assert CountPlan.get([c10], "vertex", False, wide=True).wide
    with pytest.raises(_abi.GsnError, match="k <= 9"):
        CountPlan.get([c10], "vertex", False)           # (the cache keeps wide and narrow requests apart)
    with pytest.raises(_abi.GsnError, match="k <= 16"):
        CountPlan([_el(nx.cycle_graph(17))], "vertex", False, wide=True)
    with pytest.raises(_abi.GsnError, match="3628800 automorphisms"):
        CountPlan([_el(nx.star_graph(10))], "vertex", False, wide=True)
    with pytest.raises(_abi.GsnError, match="3628800 automorphisms"):
        CountPlan([_el(nx.complete_graph(10))], "edge", False, wide=True)
    narrow = CountPlan([_el(nx.cycle_graph(k)) for k in range(3, 10)], "edge", False, wide=True)
    assert not narrow.wide and narrow.kmax == 9
    # the fused routes refuse a wide plan before they look at anything else
    from gsn_amd.counting import count_batch, count_batch_side
    from gsn_amd.step import CountLayerStep
    wide_e = CountPlan([c10], "edge", False, wide=True)
    with pytest.raises(ValueError, match="wide plans count only"):
        CountLayerStep(wide_e, None, [3])
    with pytest.raises(ValueError, match="wide plans count only"):
        count_batch_side(wide_e, None, None, None, 1, 1)
    with pytest.raises(ValueError, match="wide plans count only"):
        count_batch(wide_e, [0, 2], [0, 2], np.array([[0, 1], [1, 0]]), encode=([3], True))
    with pytest.raises(_abi.GsnError, match='large="sparse"'):
        count_batch(wide_e, [0, 2], [0, 2], np.array([[0, 1], [1, 0]]))


def _families():
    from networkx.generators.atlas import graph_atlas_g
    five = [list(g.edges) for g in graph_atlas_g() if g.number_of_nodes() == 5 and nx.is_connected(g)]
    return {
        "cycles": [list(nx.cycle_graph(k).edges) for k in range(3, 7)],
        "cliques": [list(nx.complete_graph(k).edges) for k in range(3, 6)],
        "paths": [list(nx.path_graph(k).edges) for k in range(3, 7)],
        "stars": [list(nx.star_graph(k - 1).edges) for k in range(3, 6)],
        "five": five,
        "star8": [list(nx.star_graph(8).edges)],
    }


def narrow_table_cases():
    """(key, patterns, mode, induced, directed_orbits, directed) of the tables whose SHA-256 tests/golden/plan_tables_narrow.json records:
    the pattern families of tests/test_count_sparse_cpu.py and star_graph(8) in every mode, and two directed vertex-mode lists."""
    cases = []
    for fam, pats in _families().items():
        for mode in ("vertex", "edge"):
            for induced in (False, True):
                for dirorb in (False, True):
                    cases.append(("%s/%s/induced=%d/directed_orbits=%d" % (fam, mode, induced, dirorb), pats, mode, induced, dirorb, False))
    dir_a = [[(0, 1), (1, 2), (2, 0)], [(0, 1), (1, 2)], [(0, 1), (0, 2)], [(1, 0), (2, 0)], [(0, 1), (1, 0), (1, 2)]]
    dir_b = [[(i, (i + 1) % 6) for i in range(6)], [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5)], [(0, 1), (0, 2), (0, 3), (0, 4)],
             [(i, (i + 1) % 9) for i in range(9)]]
    for name, pats in (("directed_a", dir_a), ("directed_b", dir_b)):
        for induced in (False, True):
            cases.append(("%s/vertex/induced=%d/directed" % (name, induced), pats, "vertex", induced, False, True))
    return cases


def test_narrow_tables_unchanged(lib):
    """The tables of patterns of at most nine vertices are, byte for byte, those recorded before the wide format existed -- with and
    without the wide bit."""
    from gsn_amd.counting import CountPlan
    with open(GOLDEN) as f:
        golden = json.load(f)
    cases = narrow_table_cases()
    assert sorted(golden) == sorted(c[0] for c in cases)
    for key, pats, mode, induced, dirorb, directed in cases:
        for wide in (False, True):
            plan = CountPlan(pats, mode, induced, dirorb, directed, wide=wide)
            assert not plan.wide
            assert len(plan.table) == golden[key]["words"], key
            assert hashlib.sha256(plan.table.astype("<u4").tobytes()).hexdigest() == golden[key]["sha256"], (key, wide)


def _pad10(pats):
    """the patterns and a 10-vertex cycle, so that the table is a wide one"""
    return list(pats) + [_el(nx.cycle_graph(10))]


def test_duplicate_column_and_self_loop(lib, harness):
    """Edge-mode row rules through the wide core: the last duplicate of a column holds the counts, earlier duplicates and self loops are zero
    rows (utils_graph_processing.py:142-144).  Vertex counts do not see either."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    n, ei = synth.er_graph(11, 22, 3)
    E = ei.shape[1]
    pats = _pad10(_families()["cycles"])
    ref = _oracle("edge", False, n, ei, pats)
    c = int(np.nonzero(ref.sum(1))[0][0])
    ei2 = np.concatenate([ei, ei[:, c:c + 1], np.array([[2], [2]])], axis=1)
    plan = CountPlan(pats, "edge", False, wide=True)
    assert plan.wide
    got, st = _count(harness, plan, n, ei2)
    want = np.concatenate([ref, ref[c:c + 1], np.zeros((1, ref.shape[1]), np.int64)], axis=0)
    want[c] = 0
    assert st == 0 and np.array_equal(got, want) and want[E].sum() > 0
    got_v, st_v = _count(harness, CountPlan(pats, "vertex", False, wide=True), n, ei2)
    assert st_v == 0 and np.array_equal(got_v, _oracle("vertex", False, n, ei, pats))


def test_missing_reverse_column_and_bad_index(lib, harness):
    """A column on a triangle whose reverse is no column: KeyError (utils_graph_processing.py:173); a column no match touches may lose its
    reverse; an endpoint outside the graph is a bad index."""
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan
    n, ei = synth.er_graph(11, 22, 3)
    pats = _pad10([list(nx.cycle_graph(3).edges)])
    plan = CountPlan(pats, "edge", False, wide=True)
    assert plan.wide
    ref = _oracle("edge", False, n, ei, pats)
    c = int(np.nonzero(ref[:, 0])[0][0])
    rev = int(np.nonzero((ei[0] == ei[1, c]) & (ei[1] == ei[0, c]))[0][0])
    got, st = _count(harness, plan, n, np.delete(ei, rev, axis=1))
    assert st == 1
    c0 = int(np.nonzero(ref.sum(1) == 0)[0][0])
    rev0 = int(np.nonzero((ei[0] == ei[1, c0]) & (ei[1] == ei[0, c0]))[0][0])
    ei0 = np.delete(ei, rev0, axis=1)
    got, st = _count(harness, plan, n, ei0)
    assert st == 0 and np.array_equal(got, np.delete(ref, rev0, axis=0))
    bad = ei.copy()
    bad[1, 3] = n
    assert _count(harness, plan, n, bad)[1] == 3


def test_narrow_harnesses_refuse_wide_tables(lib):
    """The magic word differs: whatever tests a table for the narrow magic refuses a wide one."""
    from gsn_amd.counting import CountPlan
    plan = CountPlan([_el(nx.cycle_graph(10))], "vertex", False, wide=True)
    assert plan.table[0] == 0x47534e32 and CountPlan([_el(nx.cycle_graph(9))], "vertex", False).table[0] == 0x47534e31
    so = os.path.join(REPO, "tests", "_build", "libsparse_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "sparse_harness.cpp")])
    out = np.zeros((4, plan.n_cols), dtype=np.int64)
    e = np.zeros(1, dtype=np.int64)
    assert ctypes.CDLL(so).sparse_harness_count(plan.table.ctypes.data_as(U32P), ctypes.c_int64(4), ctypes.c_int64(0), e.ctypes.data_as(I64P),
                                                e.ctypes.data_as(I64P), out.ctypes.data_as(I64P)) == -1


def test_other_entries_name_the_sparse_kernel(lib):
    """gsn_count_hip and the entries on it, handed a wide table, answer GSN_E_UNSUPPORTED and say which entry takes it (before any pointer
    is looked at: no device is needed)."""
    from gsn_amd import _abi
    from gsn_amd.counting import CountPlan
    plan = CountPlan([_el(nx.cycle_graph(10))], "edge", False, wide=True)
    out = np.zeros(plan.n_cols, dtype=np.int64)
    rc = lib.gsn_count_hip(_abi.ptr(plan.table), None, len(plan.table), 1, None, None, None, 0, 0, None, 1, 8, 8, _abi.ptr(out), None, None)
    assert rc == -2
    with pytest.raises(_abi.GsnError, match="wide plan .*gsn_count_sparse_hip only"):
        _abi.check(rc, "gsn_count_hip")


def test_wide_harness_under_address_and_undefined_sanitizers(lib, zinc769):
    """The wide core as a stand-alone program built with -fsanitize=address,undefined: the 16-vertex patterns on the 4-cube, the mixed table
    in edge mode with a duplicated column and a self loop, a directed table, and the 769-vertex graph."""
    from gsn_amd.counting import CountPlan
    exe = os.path.join(REPO, "tests", "_build", "sparse_wide_harness_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSPARSE_HARNESS_MAIN", "-o", exe, SRC])
    lists, tg = pattern_lists(), targets()
    n, ei = tg["ladder8"]
    ei_dup = np.concatenate([ei, ei[:, :1], np.array([[2], [2]])], axis=1)
    dpats, dgraphs = directed_cases()
    cases = [("cube", lists["cycles10_16"] + lists["paths"] + lists["binomial4"], "vertex", False, False) + tg["hypercube4"],
             ("dup", lists["mixed3_12"] + lists["trees10"], "edge", True, False, n, ei_dup),
             ("petersen", lists["petersen"] + lists["k55"] + lists["star9"], "edge", False, False) + tg["petersen_pendant"],
             ("directed", dpats, "vertex", True, True) + dgraphs[1],
             ("n769", zinc769_patterns(), "vertex", False, False) + zinc769]
    for name, pats, mode, induced, directed, n, ei in cases:
        plan = CountPlan(pats, mode, induced, False, directed, wide=True)
        assert plan.wide
        ei = np.ascontiguousarray(ei, dtype=np.int64)
        if name == "dup":
            ref = _oracle(mode, induced, n, ei[:, :-2], pats)
            want = np.concatenate([ref, ref[:1], np.zeros((1, ref.shape[1]), np.int64)], axis=0)
            want[0] = 0
        else:
            want = _oracle(mode, induced, n, ei, pats, directed=directed)
        path = os.path.join(REPO, "tests", "_build", "sparse_wide_case_%s.bin" % name)
        table = plan.table if len(plan.table) % 2 == 0 else np.concatenate([plan.table, np.zeros(1, np.uint32)])
        with open(path, "wb") as f:
            f.write(np.array([len(plan.table), n, ei.shape[1], plan.n_cols, 0], dtype=np.int64).tobytes())
            f.write(table.astype(np.uint32).tobytes())
            f.write(np.ascontiguousarray(ei[0]).tobytes() + np.ascontiguousarray(ei[1]).tobytes())
            f.write(np.ascontiguousarray(want, dtype=np.int64).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        assert r.stdout.startswith("sparse wide harness ok:")
