"""The counting launch of the headline step after its set-up was shortened (count.hip: both CSR ranks of a column in one visit, 32-bit
endpoint tests, launch-uniform flags and the side workgroups' arms as the type CycKeys, row stores through a buffer resource, the code status
cleared inside the launch).  Identifiers and status words are compared bit for bit with count_batch on the plan interpreter
(GSN_COUNT_CYCLE=0, run once in a child process: tests/count_ranks_child.py); the side outputs with build_csr_graphs and with the encoders'
definition (include/gsn_abi.h: key byte per vertex, key word per sorted column, identifier mask per column), written out in numpy here."""
import os
import re
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import torch

from count_ranks_cases import ALL_CASES, ST_BAD_INDEX, ST_KEYERROR, ST_TOO_LARGE, bad_index_status, columns_status, count_case
from step_keys_batches import make_layer

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
FLOWS = ["source_to_target", "target_to_source"]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.fixture(scope="module")
def interp(tmp_path_factory):
    """Identifiers and status words of every case from the plan interpreter: one child process for the module."""
    path = tmp_path_factory.mktemp("count_ranks") / "interp.npz"
    env = dict(os.environ, GSN_COUNT_CYCLE="0", GSN_CHAIN_TRACE="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "count_ranks_child.py"), str(path)], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "cycle walk 1" not in r.stderr and "gsn count: count_kernel<1,64>" in r.stderr
    ref = dict(np.load(str(path)))
    assert sorted(ref) == sorted(n + s for n in ALL_CASES for s in ("/ids", "/status"))
    return ref


@pytest.fixture(scope="module")
def layers_by_flow():
    return {flow: make_layer(flow, seed=1) for flow in FLOWS}


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")      # (read at every launch: the library names the instantiation it takes on stderr)


# ---- the definitions ----------------------------------------------------------------------------------------------------------------------
def _hot_bits(ids, classes, clamp):
    m, first = np.zeros(ids.shape[0], dtype=np.int64), 0
    for c, ncls in enumerate(classes):
        cls = np.minimum(ids[:, c], ncls - 1) if clamp else ids[:, c]
        ok = cls < ncls
        m[ok] |= 1 << (first + cls[ok])
        first += ncls
    return m


def _node_keys(codes, n_classes, clamp):
    """Mixed-radix number of a vertex's code digits, column 0 most significant; without clamp a column has one digit more, "none"."""
    codes = codes.reshape(codes.shape[0], -1)
    key, bad = np.zeros(codes.shape[0], dtype=np.int64), False
    for c, ncls in enumerate(n_classes):
        x = codes[:, c]
        if clamp:
            digit, radix = np.clip(x, 0, ncls - 1), ncls
        else:
            ok = (x >= 0) & (x < ncls)
            digit, radix, bad = np.where(ok, x, ncls), ncls + 1, bad or not ok.all()
        key = key * radix + digit
    return key, bad


def _edge_bits(codes, ncls, clamp):
    x = np.clip(codes, 0, ncls - 1) if clamp else codes
    ok = (x >= 0) & (x < ncls)
    return np.where(ok, 1 << np.clip(x, 0, ncls - 1), 0), not ok.all()


def _csr_definition(node_ptr, edge_ptr, ei, glob, row, lds_bytes):
    """Stable sort of the columns by target.  A side workgroup takes the graphs of four counting workgroups -- eight graphs -- and, with
    global ids, sorts as ONE disjoint union as many consecutive graphs of them as fit the launch's LDS together ((n + 1) * 8 + n * 4 +
    E * 7 + 16 bytes; count.hip: side_block): an endpoint is tested against the union's vertex range, and one outside it counts as the
    union's first vertex.  With graph-local ids a graph is sorted by itself.  (Where every endpoint lies in its graph, any grouping gives
    the same arrays.)"""
    N, E, G = int(node_ptr[-1]), int(edge_ptr[-1]), len(node_ptr) - 1
    seg, perm, tgt, oth = np.zeros(N + 1, np.int64), np.zeros(E, np.int64), np.zeros(E, np.int64), np.zeros(E, np.int64)
    seg[N] = E
    bounds = [0]
    while bounds[-1] < G:
        g = bounds[-1]
        g1, end = g + 1, min(G, (g // 8 + 1) * 8)
        need = lambda h: (node_ptr[h] - node_ptr[g] + 1) * 8 + (node_ptr[h] - node_ptr[g]) * 4 + (edge_ptr[h] - edge_ptr[g]) * 7 + 16
        while glob and g1 < end and need(g1 + 1) <= lds_bytes:
            g1 += 1
        bounds.append(g1)
    for g, g1 in zip(bounds[:-1], bounds[1:]):
        n0, n, e0, e1 = int(node_ptr[g]), int(node_ptr[g1] - node_ptr[g]), int(edge_ptr[g]), int(edge_ptr[g1])
        loc = ei[:, e0:e1] - (n0 if glob else 0)
        loc = np.where((loc >= 0) & (loc < n), loc, 0)
        order = np.argsort(loc[row], kind="stable")
        perm[e0:e1], tgt[e0:e1], oth[e0:e1] = e0 + order, n0 + loc[row][order], n0 + loc[1 - row][order]
        seg[n0:n0 + n] = e0 + np.searchsorted(loc[row][order], np.arange(n), side="left")
    return seg, perm, tgt, oth


def _codes(N, E, seed, node_classes=(28,), edge_classes=(4,), node_over=0, edge_over=0):
    """Random codes; `node_over` / `edge_over` > 0: some codes lie that far beyond their classes (and some below zero)."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, c, N) for c in node_classes], axis=1).astype(np.int64)
    e = np.stack([rng.integers(0, c, E) for c in edge_classes], axis=1).astype(np.int64)
    if node_over:
        x[::7, 0] = node_classes[0] + node_over - 1
        x[3::11, -1] = -2
    if edge_over:
        e[::5, 0] = edge_classes[0] + edge_over - 1
        e[2::13, 0] = -1
    return (x[:, 0] if len(node_classes) == 1 else x), (e[:, 0] if len(edge_classes) == 1 else e)


def _run(capfd, layer, name, interp, flags_type="CycKeys", classes=(3, 3, 3, 3), clamp=True, node_classes=(28,), node_clamp=True, edge_clamp=True,
         node_over=0, edge_over=0, want_status=None):
    """One CountLayerStep over a named case; asserts every output of the counting launch.  Returns the stepper."""
    from gsn_amd import layers
    from gsn_amd._index import build_csr_graphs
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    node_ptr, edge_ptr, ei, glob, mn, me = count_case(name)
    N, E = int(node_ptr[-1]), int(edge_ptr[-1])
    x, ef = _codes(N, E, E, node_classes=node_classes, node_over=node_over, edge_over=edge_over)
    xc, efc = layers.Codes(_t(x), list(node_classes), clamp=node_clamp, check=False), layers.Codes(_t(ef), [4], clamp=edge_clamp, check=False)
    step = CountLayerStep(CountPlan.get(CYCLES, "edge", False), layer, list(classes), clamp=clamp)
    capfd.readouterr()
    ids, y, status = step(_t(node_ptr), _t(edge_ptr), _t(ei), xc, efc, mn, me, ids_are_global=glob)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert step.on_keys and "cycle walk 1" in err and "cycle flags " + flags_type in err
    # identifiers and status words: the interpreter's
    want_ids, want_st = interp[name + "/ids"], interp[name + "/status"]
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(status.cpu().numpy(), want_st)
    if want_status is not None:
        assert want_st.tolist() == list(want_status)
    b = step._bufs[1]
    bits = _hot_bits(want_ids, classes, clamp)
    for g in np.flatnonzero(want_st >= ST_TOO_LARGE):                   # (reported, not counted: no class bit)
        bits[edge_ptr[g]:edge_ptr[g + 1]] = 0
    assert np.array_equal(b["idmask"][:E].cpu().numpy().astype(np.int64) & 0xffff, bits)
    # the side outputs: the CSR by its definition and, where every column stays inside its graph, by build_csr_graphs
    row = layer._sel()
    seg, perm, tgt, oth = _csr_definition(node_ptr, edge_ptr, ei, glob, row, int(re.search(r"count_kernel<1,64> workgroups \d+ pair 1 split 1 lds (\d+)", err).group(1)))
    c = step.csr()
    got = [a.cpu().numpy().astype(np.int64) for a in (c.seg_ptr, c.perm[:E], c.tgt[:E], c.src[:E])]
    nkey, bad_n = _node_keys(x, node_classes, node_clamp)
    assert np.array_equal(b["nkey"].cpu().numpy().astype(np.int64), nkey)
    for a, w in zip(got, (seg, perm, tgt, oth)):
        assert np.array_equal(a, w)
    if not (want_st == ST_BAD_INDEX).any():              # (build_csr_graphs refuses a batch whose columns leave their graphs)
        eig = _t(ei + (np.repeat(node_ptr[:-1], np.diff(edge_ptr))[None, :] if not glob else 0))
        ref = build_csr_graphs(eig[row], N, _t(node_ptr), _t(edge_ptr), mn, me, other=eig[1 - row], check=True)
        for a, w in zip((c.seg_ptr, c.perm[:E], c.tgt[:E], c.src[:E]), ref):
            assert torch.equal(a, w)
    ebit, bad_e = _edge_bits(ef, 4, edge_clamp)
    ekeys = nkey[tgt] | (nkey[oth] << 8) | (ebit[perm] << 16)
    assert np.array_equal(b["ekeys"][:E].cpu().numpy().astype(np.int64) & 0xffffffff, ekeys)
    assert int(b["code_status"].item()) == int(bad_n or bad_e)
    return step


# ---- size edges, columns, indices and ids, both csr_row values -------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("name", ["size_edges", "size_edges_local"])
def test_trips_of_64_columns_one_vertex_a_self_loop_64_vertices_and_pairs_redone_alone(capfd, interp, layers_by_flow, name, flow):
    layer = layers_by_flow[flow]
    assert layer._sel() == (1 if flow == "source_to_target" else 0)
    _run(capfd, layer, name, interp, flags_type="CycKeys" if name == "size_edges" else "CycAny")
    ids = interp[name + "/ids"]
    assert (ids.max(axis=0) > 0).all() and interp[name + "/status"].max() == 0
    node_ptr, edge_ptr = count_case(name)[:2]
    assert 64 in np.diff(node_ptr) and 1 in np.diff(node_ptr) and 0 in np.diff(edge_ptr)


@pytest.mark.parametrize("name", ["columns", "columns_local"])
def test_a_column_three_times_and_a_pair_in_one_direction_only(capfd, interp, layers_by_flow, name):
    _run(capfd, layers_by_flow[FLOWS[0]], name, interp, flags_type="CycKeys" if name == "columns" else "CycAny", want_status=columns_status())
    ids, (node_ptr, edge_ptr, ei) = interp[name + "/ids"], count_case(name)[:3]
    first = ei[:, :int(edge_ptr[1])]
    same = np.flatnonzero((first[0] == first[0][0]) & (first[1] == first[1][0]))
    assert len(same) == 4 and not ids[same[:-1]].any() and ids[same[-1]].any()       # the last duplicate carries the counts
    assert ids[int(edge_ptr[1]):int(edge_ptr[2])].any()                             # the one-way graph's rows are counted


@pytest.mark.parametrize("name", ["one_way", "one_way_local"])
def test_graphs_whose_pairs_all_come_in_one_direction(capfd, interp, layers_by_flow, name):
    """Twice as many slots of the CSR rank as columns: every slot is cleared, a pair with more slots than its table holds is redone alone."""
    from count_ranks_cases import one_way_status
    _run(capfd, layers_by_flow[FLOWS[0]], name, interp, flags_type="CycKeys" if name == "one_way" else "CycAny", want_status=one_way_status())
    ids, edge_ptr = interp[name + "/ids"], count_case(name)[1]
    assert ids[int(edge_ptr[2]):int(edge_ptr[3]), 2].all() and ids[int(edge_ptr[4]):int(edge_ptr[5])].any()   # the ring's 5-cycle; the two-way graph
    assert not ids[:int(edge_ptr[2])].any()


@pytest.mark.parametrize("name", ["bad_index", "bad_index_local"])
def test_endpoints_at_minus_one_at_n_and_beyond_32_bits(capfd, interp, layers_by_flow, name):
    _run(capfd, layers_by_flow[FLOWS[0]], name, interp, flags_type="CycKeys" if name == "bad_index" else "CycAny", want_status=bad_index_status())
    ids, st, edge_ptr = interp[name + "/ids"], interp[name + "/status"], count_case(name)[1]
    for g in range(len(st)):
        rows = ids[int(edge_ptr[g]):int(edge_ptr[g + 1])]
        assert rows.any() == (st[g] == 0)                                           # zero rows where reported, counts beside them


# ---- node and edge codes -----------------------------------------------------------------------------------------------------------------------
def test_two_node_code_columns_take_the_generic_flags(capfd, interp, layers_by_flow):
    layer = layers_by_flow[FLOWS[0]]                 # (28 node columns: 12 + 16 classes; 192 / 221 dictionary rows)
    _run(capfd, layer, "size_edges", interp, flags_type="CycAny", node_classes=(12, 16))
    _run(capfd, layer, "columns", interp, flags_type="CycAny", node_classes=(12, 16), node_clamp=False, node_over=2)


@pytest.mark.parametrize("clamp", [True, False])
def test_codes_outside_their_classes(capfd, interp, layers_by_flow, clamp):
    """Clamped: the last (or first) class, no status.  Not clamped: the "none" digit / no edge bit, and the code status."""
    step = _run(capfd, layers_by_flow[FLOWS[1]], "size_edges", interp, node_clamp=clamp, edge_clamp=clamp, node_over=3, edge_over=2)
    assert int(step._bufs[1]["code_status"].item()) == (0 if clamp else 1)


# ---- the code status is the launch's ----------------------------------------------------------------------------------------------------------
def _status_step(layer, bad):
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    node_ptr, edge_ptr, ei, glob, mn, me = count_case("size_edges")
    N, E = int(node_ptr[-1]), int(edge_ptr[-1])
    x, ef = _codes(N, E, 5)
    xt, et = _t(x), _t(ef)
    if bad:
        et[E - 1] = 9
    step = CountLayerStep(CountPlan.get(CYCLES, "edge", False), layer, [3, 3, 3, 3])
    xc, efc = layers.Codes(xt, [28], clamp=False, check=False), layers.Codes(et, [4], clamp=False, check=False)
    args = (_t(node_ptr), _t(edge_ptr), _t(ei), xc, efc, mn, me)
    return step, args, et, E


def test_a_clean_step_after_a_bad_code_step_reads_clean(layers_by_flow):
    step, args, et, E = _status_step(layers_by_flow[FLOWS[0]], bad=True)
    step(*args)
    with pytest.raises(IndexError):
        step.check_status()
    et[E - 1] = 1                                    # the same buffers, the same stepper: only the code is valid now
    step(*args)
    step.check_status()
    assert int(step._bufs[1]["code_status"].item()) == 0


def test_a_clean_replay_after_a_bad_code_replay_reads_clean(layers_by_flow):
    from gsn_amd.graphs import GraphedStep
    step, args, et, E = _status_step(layers_by_flow[FLOWS[0]], bad=False)
    ids_g, y_g, _ = step(*args)
    graphed = GraphedStep(lambda: step(*args, ids_out=ids_g, out=y_g), warmup=1)
    graphed()
    step.check_status()
    et[E - 1] = 9
    graphed()
    with pytest.raises(IndexError):
        step.check_status()
    et[E - 1] = 2
    graphed()
    step.check_status()


# ---- a molecule batch ---------------------------------------------------------------------------------------------------------------------------
def test_2000_molecules_equal_the_composition(capfd, interp, layers_by_flow):
    """ids, y, csr() and packs() of the one-call step against counting (the interpreter's identifiers), build_csr_graphs, the pack encoders
    and the plain layer call on integer codes."""
    from gsn_amd import layers, packs, synth
    layer = layers_by_flow[FLOWS[0]]
    b = synth.zinc_shape_batch(2000, seed=11)
    node_ptr, edge_ptr, ei, glob, mn, me = count_case("zinc")
    assert np.array_equal(ei, b.edge_index)
    N, E = b.num_nodes, b.num_edges
    want_ids = interp["zinc/ids"]
    assert interp["zinc/status"].max() == 0 and (want_ids.max(axis=0) > 0).all()
    from gsn_amd._index import build_csr_graphs
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    xc, efc = layers.Codes(_t(b.atom_type), [28]), layers.Codes(_t(b.bond_type), [4])
    step = CountLayerStep(CountPlan.get(CYCLES, "edge", False), layer, [3, 3, 3, 3], clamp=True)
    capfd.readouterr()
    eit = _t(ei)
    ids, y, status = step(_t(node_ptr), _t(edge_ptr), eit, xc, efc, mn, me)
    step.check_status()
    assert step.on_keys and "cycle flags CycKeys" in capfd.readouterr().err
    assert np.array_equal(ids.cpu().numpy(), want_ids) and int(status.abs().sum()) == 0
    c = step.csr()
    ref = build_csr_graphs(eit[layer._sel()], N, _t(node_ptr), _t(edge_ptr), mn, me, other=eit[1 - layer._sel()], check=True)
    for a, w in zip((c.seg_ptr, c.perm[:E], c.tgt[:E], c.src[:E]), ref):
        assert torch.equal(a, w)
    npk, epk = step.packs()
    assert torch.equal(npk.view(torch.int16), packs.pack_node_codes(layers.Codes(_t(b.atom_type), [28])).view(torch.int16))
    hot = _hot_bits(want_ids, [3, 3, 3, 3], True) | (1 << (12 + b.bond_type.astype(np.int64)))
    want_epk = ((hot[:, None] >> np.arange(16)[None, :]) & 1).astype(np.float16)
    assert np.array_equal(epk[:E].cpu().numpy().view(np.int16), want_epk.view(np.int16))
    with torch.no_grad():
        y_ref = layer(layers.Codes(_t(b.atom_type), [28]), eit, identifiers=layers.Codes(_t(want_ids), [3, 3, 3, 3], clamp=True),
                      degrees=torch.zeros(N, device=_dev()), edge_features=layers.Codes(_t(b.bond_type), [4]))
    assert torch.equal(y, y_ref)
