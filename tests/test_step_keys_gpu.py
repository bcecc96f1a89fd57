"""The key path of the one-call step (gsn_count_layer_step_keys_hip, gsn_amd.step.CountLayerStep): the counting launch leaves key bytes, key
words and identifier masks instead of the two row packs, layer 0 gathers its operand rows from the node dictionary and the byte table.
Against the pack path (``force_packs=True``: gsn_count_layer_step_hip) everything must be equal bit for bit -- int64 identifiers, layer rows,
status words, CSR arrays -- and the compact outputs must be what include/gsn_abi.h defines them to be."""
import os

import numpy as np
import pytest
import torch

from step_keys_batches import collate_to_device, cycles, hand_made_graphs, make_layer

pytestmark = pytest.mark.gpu
no_cache = pytest.mark.skipif(os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING") == "1",
                              reason="stream capture cannot free memory without the caching allocator (scripts/oob_check.sh)")
FLOWS = ["source_to_target", "target_to_source"]


def _dev():
    return torch.device("cuda", 0)


def _zinc(n_graphs, seed):
    from gsn_amd import synth
    b = synth.zinc_shape_batch(n_graphs, seed=seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return b, t(b.node_ptr), t(b.edge_ptr), t(b.edge_index), t(b.atom_type), t(b.bond_type)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _both(plan, layer, id_classes, node_ptr, edge_ptr, ei, xc, efc, mn, me, expect_keys=True):
    """One step on each path; asserts every output equal and returns (key-path stepper, ids, y)."""
    from gsn_amd.step import CountLayerStep
    sk = CountLayerStep(plan, layer, id_classes, clamp=True)
    sp = CountLayerStep(plan, layer, id_classes, clamp=True, force_packs=True)
    ids_k, y_k, st_k = sk(node_ptr, edge_ptr, ei, xc, efc, mn, me)
    ids_p, y_p, st_p = sp(node_ptr, edge_ptr, ei, xc, efc, mn, me)
    torch.cuda.synchronize()
    assert sk.on_keys == expect_keys and not sp.on_keys
    assert torch.equal(ids_k, ids_p)
    assert torch.equal(_bits(y_k), _bits(y_p))
    assert torch.equal(st_k, st_p)
    assert torch.equal(sk._bufs[1]["code_status"], sp._bufs[1]["code_status"])
    ck, cp = sk.csr(), sp.csr()
    for a, b in ((ck.seg_ptr, cp.seg_ptr), (ck.perm, cp.perm), (ck.tgt, cp.tgt), (ck.src, cp.src)):
        assert torch.equal(a, b)
    nk, ek = sk.packs()
    npk, epk = sp.packs()
    assert torch.equal(nk.view(torch.int16), npk.view(torch.int16)) and torch.equal(ek.view(torch.int16), epk.view(torch.int16))
    return sk, ids_k, y_k


def _zinc_case(n_graphs, flow, seed):
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(n_graphs, seed)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer(flow)
    xc, efc = layers.Codes(atoms, [28]), layers.Codes(bonds, [4])
    sk, ids, y = _both(plan, layer, [3, 3, 3, 3], node_ptr, edge_ptr, ei, xc, efc, mn, me)
    assert int(sk._bufs[1]["status"].abs().sum()) == 0 and int(sk._bufs[1]["code_status"].item()) == 0
    return b, sk, ids, atoms, bonds


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("n_graphs", [1, 2, 9, 41])
def test_key_step_equals_pack_step_on_molecules(n_graphs, flow):
    """(a) G = 9: one full side workgroup and a partial one; G = 41: ~30 tiles."""
    _zinc_case(n_graphs, flow, 300 + n_graphs)


def test_key_step_equals_pack_step_when_waves_walk_two_tiles():
    """(b) ~2 200 tiles for 2 048 wave ranges: the gathers issued across a tile boundary."""
    b, sk, ids, atoms, bonds = _zinc_case(3000, "source_to_target", 17)
    assert (b.num_nodes + 31) // 32 > 2048


def _hand_made(flow, n_cycle_cols, id_classes):
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    graphs = hand_made_graphs()
    b, node_ptr, edge_ptr, ei = collate_to_device(graphs)
    N, E = b.num_nodes, b.num_edges
    assert E % 32 != 0
    rng = np.random.default_rng(3)
    atoms = torch.from_numpy(rng.integers(0, 28, N)).to(_dev())
    bonds = torch.from_numpy(rng.integers(0, 4, E)).to(_dev())
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    plan = CountPlan.get(cycles(range(3, 3 + n_cycle_cols)), "edge", False)
    layer = make_layer(flow, seed=3)
    sk, ids, y = _both(plan, layer, id_classes, node_ptr, edge_ptr, ei, layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), mn, me)
    return b, sk, ids, atoms, bonds


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("n_cycle_cols,id_classes", [(4, [3, 3, 3, 3]), (3, [4, 4, 4])])
def test_key_step_equals_pack_step_on_hand_made_multigraphs(flow, n_cycle_cols, id_classes):
    """(c) a vertex with no in-edge, a tile whose only block is empty, a hub of in-degree 70, E no multiple of 32, duplicate columns, self
    loops; four cycle columns (the cycle instantiation) and three (the generic one: the general arm of the encoded rows)."""
    b, sk, ids, atoms, bonds = _hand_made(flow, n_cycle_cols, id_classes)
    deg = np.bincount(b.edge_index[1 if flow == "source_to_target" else 0], minlength=b.num_nodes)
    assert deg.max() == 70 and (deg == 0).sum() >= 60


def test_key_step_equals_pack_step_on_the_molecule_instantiation():
    """Four columns that are not all short cycles (a 7-cycle keeps the plan interpreter): the molecule instantiation's identifier masks."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(9, 51)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    plan = CountPlan.get(cycles([3, 5, 6, 7]), "edge", False)
    _both(plan, make_layer("source_to_target"), [3, 3, 3, 3], node_ptr, edge_ptr, ei, layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), mn, me)


def _hot_mask(values, n_classes, clamp, col0=0):
    """Bit mask of the hot columns of one-hot(values) over consecutive class blocks starting at col0 (values int64 [R, C])."""
    m = torch.zeros(values.shape[0], dtype=torch.int64, device=values.device)
    lo = col0
    for c, ncls in enumerate(n_classes):
        x = values[:, c].clamp(0, ncls - 1) if clamp else values[:, c]
        ok = (x >= 0) & (x < ncls)
        m |= torch.where(ok, torch.ones_like(x) << (lo + x.clamp(0, ncls - 1)), torch.zeros_like(x))
        lo += ncls
    return m


def _check_definitions(sk, ids, x_codes, ef_codes, id_classes):
    """(d) the compact outputs of the last step of ``sk`` against their definitions, computed with torch."""
    from gsn_amd import packs
    from gsn_amd.step import node_key
    b = sk._bufs[1]
    E = ids.shape[0]
    nkey = b["nkey"].long()
    assert torch.equal(nkey, node_key(x_codes.codes, x_codes.n_classes, x_codes.clamp))
    perm, tgt, src = b["perm"][:E].long(), b["tgt"][:E].long(), b["src"][:E].long()
    bond = _hot_mask(ef_codes.codes, ef_codes.n_classes, ef_codes.clamp)
    assert torch.equal(b["ekeys"][:E].long(), nkey[tgt] | (nkey[src] << 8) | (bond[perm] << 16))
    assert torch.equal(b["idmask"][:E].long() & 0xffff, _hot_mask(ids, id_classes, True))
    npk, epk = sk.packs()
    ref = packs.pack_node_codes(type(x_codes)(x_codes.codes.clone(), x_codes.n_classes, clamp=x_codes.clamp, check=False))      # gsn_one_hot_pack16_hip
    assert torch.equal(npk.view(torch.int16), ref.view(torch.int16))
    w = sum(id_classes)
    one_hot = torch.cat([torch.nn.functional.one_hot(ids[:, c].clamp(max=n - 1), n) for c, n in enumerate(id_classes)], 1)
    assert torch.equal(epk[:, :w].long(), one_hot)
    bits = (bond.unsqueeze(1) >> torch.arange(16 - w, device=bond.device).unsqueeze(0)) & 1
    assert torch.equal(epk[:, w:].long(), bits)


def test_compact_outputs_are_what_the_header_defines():
    from gsn_amd import layers
    b, sk, ids, atoms, bonds = _zinc_case(41, "source_to_target", 341)
    _check_definitions(sk, ids, layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), [3, 3, 3, 3])
    b, sk, ids, atoms, bonds = _hand_made("target_to_source", 3, [4, 4, 4])
    _check_definitions(sk, ids, layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), [4, 4, 4])


@pytest.mark.parametrize("id_classes,bond_classes", [([2, 2, 2, 2], 8), ([2, 2, 4, 4], 4)])
def test_class_layouts_that_move_the_half_row_boundary(id_classes, bond_classes):
    """(e) identifier classes end at column 8 (the lane halves split exactly between identifiers and bond classes) / at column 12 with classes
    of unequal width; the bond classes fill the row."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(9, 77)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    bonds = torch.from_numpy(np.random.default_rng(1).integers(0, bond_classes, b.num_edges)).to(_dev())
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", d_ef=bond_classes, d_id=sum(id_classes))
    xc, efc = layers.Codes(atoms, [28]), layers.Codes(bonds, [bond_classes])
    sk, ids, y = _both(plan, layer, id_classes, node_ptr, edge_ptr, ei, xc, efc, mn, me)
    _check_definitions(sk, ids, xc, efc, id_classes)


def test_sixteen_columns_bound_both_paths_alike():
    """Identifier classes [2, 2, 4, 4] with 8 bond classes are 20 edge-level columns: beyond the 16 of an edge pack row and of the mask, refused
    by the constructor's own check on either path."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(2, 5)
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", d_ef=8, d_id=12)
    for force in (False, True):
        step = CountLayerStep(plan, layer, [2, 2, 4, 4], force_packs=force)
        with pytest.raises(ValueError, match="code widths outside the packs"):
            step(node_ptr, edge_ptr, ei, layers.Codes(atoms, [28]), layers.Codes(bonds, [8]), 40, 100)


@pytest.mark.parametrize("clamp", [True, False])
def test_two_node_code_columns(clamp):
    """(e) node codes [7, 5] (the layer kernel takes node widths that are multiples of 4: [7, 4] = 11 columns is refused on either path): a
    dictionary of 35 rows (clamped: codes above the last class count as it) or 8 x 6 = 48 with the "none" digits."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(9, 78)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    rng = np.random.default_rng(2)
    hi = (9, 7) if clamp else (7, 5)
    codes = torch.from_numpy(np.stack([rng.integers(0, hi[0], b.num_nodes), rng.integers(0, hi[1], b.num_nodes)], 1)).to(_dev())
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("target_to_source", d_in=12)
    xc, efc = layers.Codes(codes, [7, 5], clamp=clamp), layers.Codes(bonds, [4])
    sk, ids, y = _both(plan, layer, [3, 3, 3, 3], node_ptr, edge_ptr, ei, xc, efc, mn, me)
    assert sk._dict.shape[0] == (35 if clamp else 48)
    _check_definitions(sk, ids, xc, efc, [3, 3, 3, 3])


def test_codes_outside_their_classes_without_clamp():
    """(e) one node code and one bond code out of range, clamp off: their segments are zero and the code status is raised, on both paths."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(9, 79)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    rng = np.random.default_rng(4)
    codes = np.stack([rng.integers(0, 7, b.num_nodes), rng.integers(0, 5, b.num_nodes)], 1)
    codes[5, 1] = 5
    bonds_np = np.asarray(b.bond_type).copy()
    bonds_np[11] = 9
    codes, bonds = torch.from_numpy(codes).to(_dev()), torch.from_numpy(bonds_np).to(_dev())
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", d_in=12)
    xc, efc = layers.Codes(codes, [7, 5], clamp=False, check=False), layers.Codes(bonds, [4], clamp=False, check=False)
    sk, ids, y = _both(plan, layer, [3, 3, 3, 3], node_ptr, edge_ptr, ei, xc, efc, mn, me)
    assert int(sk._bufs[1]["code_status"].item()) == 1
    npk, epk = sk.packs()
    assert bool((npk[5, 7:12] == 0).all()) and float(npk[5, :7].sum()) == 1 and bool((epk[11, 12:] == 0).all())
    _check_definitions(sk, ids, xc, efc, [3, 3, 3, 3])


def test_a_dictionary_beyond_256_rows_takes_the_pack_path(monkeypatch, capfd):
    """(f) node codes [7, 7, 6]: 294 rows do not fit a key byte -- the step runs on packs, as the launch trace and the results show."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(9, 80)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    codes = torch.from_numpy(np.random.default_rng(6).integers(0, 6, (b.num_nodes, 3))).to(_dev())
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", d_in=20)
    xc, efc = layers.Codes(codes, [7, 7, 6], clamp=True), layers.Codes(bonds, [4])
    capfd.readouterr()
    _both(plan, layer, [3, 3, 3, 3], node_ptr, edge_ptr, ei, xc, efc, mn, me, expect_keys=False)
    err = capfd.readouterr().err
    assert "layer_fused_kernel_rp<4,2> nodes" in err and "layer_fused_kernel_rp<4,2> keys" not in err
    # and the trace does name the key kernel where it runs
    step = CountLayerStep(plan, make_layer("source_to_target"), [3, 3, 3, 3])
    step(node_ptr, edge_ptr, ei, layers.Codes(atoms, [28]), efc, mn, me)
    torch.cuda.synchronize()
    assert step.on_keys and "layer_fused_kernel_rp<4,2> keys" in capfd.readouterr().err


@no_cache
def test_key_step_is_capturable_and_replays_on_refilled_inputs():
    """(g) as the pack path's capture test: the replay reads the codes again, nothing input-keyed is cached."""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    b, node_ptr, edge_ptr, ei, atoms, bonds = _zinc(128, 77)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    dev = _dev()
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", seed=2)
    xc, efc = layers.Codes(atoms, [28]), layers.Codes(bonds, [4])
    step = CountLayerStep(plan, layer, [3, 3, 3, 3])
    ids0, y0, _ = step(node_ptr, edge_ptr, ei, xc, efc, mn, me)
    assert step.on_keys
    ids_g, y_g = torch.empty_like(ids0), torch.empty_like(y0)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        step(node_ptr, edge_ptr, ei, xc, efc, mn, me, ids_out=ids_g, out=y_g)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(node_ptr, edge_ptr, ei, xc, efc, mn, me, ids_out=ids_g, out=y_g)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ids_g, ids0) and torch.equal(y_g, y0)
    atoms.copy_((atoms + 3) % 28); bonds.copy_((bonds + 1) % 4)
    g.replay()
    ids1, y1, _ = step(node_ptr, edge_ptr, ei, xc, efc, mn, me)
    torch.cuda.synchronize()
    assert torch.equal(ids_g, ids1) and torch.equal(y_g, y1) and not torch.equal(y1, y0)
    pk = CountLayerStep(plan, layer, [3, 3, 3, 3], force_packs=True)
    ids2, y2, _ = pk(node_ptr, edge_ptr, ei, xc, efc, mn, me)
    assert torch.equal(ids1, ids2) and torch.equal(_bits(y1), _bits(y2))
