"""The table arm of the key path (gsn_count_layer_step_tabs_hip, csrc/layer_rp.hip TABS): the edge stage's accumulators start from the table
row of the row's target (the x_i chunks' products, made once per prepared weight set by gsn_layer_key_tables_hip with the kernel's own
instruction sequence) and only the remaining three chunks are multiplied.  Every case is one ``CountLayerStep`` on tables against the same
step on packs (``force_packs=True``) and against the KEYS arm (``GSN_RP_TABLES=0``): layer rows bit for bit, identifiers, statuses, CSR.

The gate is the dictionary's row count alone (<= 31).  A table for node stage 0's [x | deg] chunks is NOT built: its gate would be a zero
degree column of the folded weight, and that column is W3a b2 -- non-zero for every msg_fn with a bias, the benchmark's layer included --
so the cases with non-zero degree columns (all of them here: make_layer's weights are random) run ON tables and must equal the packs."""
import os

import numpy as np
import pytest
import torch

from step_keys_batches import collate_to_device, cycles, hand_made_graphs, make_layer

pytestmark = pytest.mark.gpu
no_cache = pytest.mark.skipif(os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING") == "1",
                              reason="stream capture cannot free memory without the caching allocator (scripts/oob_check.sh)")
TAB = "layer_fused_kernel_rp<4,2> keys nodes"


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _zinc(n_graphs, seed):
    from gsn_amd import synth
    b = synth.zinc_shape_batch(n_graphs, seed=seed)
    return b, (_t(b.node_ptr), _t(b.edge_ptr), _t(b.edge_index)), _t(b.atom_type), _t(b.bond_type)


def _sizes(b):
    return int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())


def _three(monkeypatch, capfd, plan, layer, id_classes, ptrs, xc, efc, mn, me, expect_tables=True):
    """One step per arm (tables / KEYS arm forced by the switch / packs): everything equal; the launch trace says which kernel arm ran."""
    from gsn_amd.step import CountLayerStep
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")
    monkeypatch.delenv("GSN_RP_TABLES", raising=False)
    st = CountLayerStep(plan, layer, id_classes, clamp=True)
    capfd.readouterr()
    ids_t, y_t, s_t = st(*ptrs, xc, efc, mn, me)
    torch.cuda.synchronize()
    line = [ln for ln in capfd.readouterr().err.splitlines() if TAB in ln]
    assert st.on_keys and st.on_tables == expect_tables
    assert len(line) == 1 and line[0].endswith(" x_i tables") == expect_tables, line
    monkeypatch.setenv("GSN_RP_TABLES", "0")
    sk = CountLayerStep(plan, layer, id_classes, clamp=True)
    ids_k, y_k, s_k = sk(*ptrs, xc, efc, mn, me)
    torch.cuda.synchronize()
    line = [ln for ln in capfd.readouterr().err.splitlines() if TAB in ln]
    assert sk.on_keys and not sk.on_tables and len(line) == 1 and not line[0].endswith(" x_i tables")
    monkeypatch.delenv("GSN_RP_TABLES")
    sp = CountLayerStep(plan, layer, id_classes, clamp=True, force_packs=True)
    ids_p, y_p, s_p = sp(*ptrs, xc, efc, mn, me)
    torch.cuda.synchronize()
    assert not sp.on_keys and not sp.on_tables
    for ids_o, y_o, s_o, so in ((ids_k, y_k, s_k, sk), (ids_p, y_p, s_p, sp)):
        assert torch.equal(ids_t, ids_o) and torch.equal(s_t, s_o)
        assert torch.equal(_bits(y_t), _bits(y_o))
        assert torch.equal(st._bufs[1]["code_status"], so._bufs[1]["code_status"])
        ct, co = st.csr(), so.csr()
        for a, b in ((ct.seg_ptr, co.seg_ptr), (ct.perm, co.perm), (ct.tgt, co.tgt), (ct.src, co.src)):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(y_t).all())
    return st, ids_t, y_t


def _zinc_case(monkeypatch, capfd, n_graphs, seed, flow="source_to_target"):
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, ptrs, atoms, bonds = _zinc(n_graphs, seed)
    plan = CountPlan.get(cycles(), "edge", False)
    return b, _three(monkeypatch, capfd, plan, make_layer(flow), [3, 3, 3, 3], ptrs, layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), *_sizes(b))


@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
@pytest.mark.parametrize("n_graphs", [1, 7])
def test_tables_equal_packs_on_molecules(n_graphs, flow, monkeypatch, capfd):
    """one graph: a single tile, a partial block (lanes past ne and nn); seven: a few tiles"""
    _zinc_case(monkeypatch, capfd, n_graphs, 500 + n_graphs, flow)


def test_tables_equal_packs_when_waves_walk_two_tiles(monkeypatch, capfd):
    """~2 200 tiles for 2 048 wave ranges: the gathers issued across a tile boundary"""
    b, _ = _zinc_case(monkeypatch, capfd, 3000, 17)
    assert (b.num_nodes + 31) // 32 > 2048


@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_tables_equal_packs_on_hand_made_multigraphs(flow, monkeypatch, capfd):
    """isolated vertices and a tile whose only block is empty (the arm without edges); a hub of in-degree 70: a tile of three blocks, both
    gather sets take turns; E no multiple of 32"""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, *ptrs = collate_to_device(hand_made_graphs())
    deg = np.bincount(b.edge_index[1 if flow == "source_to_target" else 0], minlength=b.num_nodes)
    assert deg.max() == 70 and (deg == 0).sum() >= 60 and b.num_edges % 32 != 0
    rng = np.random.default_rng(3)
    atoms, bonds = _t(rng.integers(0, 28, b.num_nodes)), _t(rng.integers(0, 4, b.num_edges))
    plan = CountPlan.get(cycles(), "edge", False)
    _three(monkeypatch, capfd, plan, make_layer(flow, seed=3), [3, 3, 3, 3], tuple(ptrs), layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), *_sizes(b))


def test_twenty_nine_rows_with_the_none_digit(monkeypatch, capfd):
    """28 atom classes without clamp: 29 dictionary rows, the last one ("none": a code outside the classes) with an all-zero x part"""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    b, ptrs, atoms, bonds = _zinc(7, 81)
    atoms = atoms.clone()
    atoms[3] = 28; atoms[-1] = 40
    plan = CountPlan.get(cycles(), "edge", False)
    xc = layers.Codes(atoms, [28], clamp=False, check=False)
    st, ids, y = _three(monkeypatch, capfd, plan, make_layer("source_to_target"), [3, 3, 3, 3], ptrs, xc, layers.Codes(bonds, [4]), *_sizes(b))
    assert st._dict.shape[0] == 29 and int(st._bufs[1]["code_status"].item()) == 1
    assert int(st._bufs[1]["nkey"][3]) == 28 and bool((st._dict[28, :28] == 0).all())


@pytest.mark.parametrize("n_classes,clamp,rows,tables", [([1, 5, 6], True, 30, True), ([4, 8], True, 32, False), ([5, 7], False, 48, False)])
def test_code_columns_at_the_row_limit(n_classes, clamp, rows, tables, monkeypatch, capfd):
    """30 rows run on tables -- the most a dictionary below the limit can have: 31 is prime, and a single column of 31 digits is wider than
    the node pack's 28 columns (tests/test_layer_key_tables_cpu.py holds the 31 / 32 cases of the gate itself); 32 rows and 48 (with the "none"
    digits) run the KEYS arm, report on_tables False and still equal the packs"""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import tables_path_ok
    b, ptrs, atoms, bonds = _zinc(7, 82)
    rng = np.random.default_rng(rows)
    codes = _t(np.stack([rng.integers(0, c, b.num_nodes) for c in n_classes], 1))
    assert tables_path_ok(n_classes, clamp) == tables
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", d_in=sum(n_classes))
    xc = layers.Codes(codes, n_classes, clamp=clamp)
    st, ids, y = _three(monkeypatch, capfd, plan, layer, [3, 3, 3, 3], ptrs, xc, layers.Codes(bonds, [4]), *_sizes(b), expect_tables=tables)
    assert st._dict.shape[0] == rows
    assert len(torch.unique(st._bufs[1]["nkey"])) > rows // 2


def test_tables_follow_the_weights(monkeypatch, capfd):
    """a weight changed in place, then a state dict loaded: the step's next call rebuilds prepared weights and tables (no stale table) --
    each time against a fresh pack-path step"""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    b, ptrs, atoms, bonds = _zinc(7, 83)
    mn, me = _sizes(b)
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", seed=5)
    xc, efc = layers.Codes(atoms, [28]), layers.Codes(bonds, [4])
    st = CountLayerStep(plan, layer, [3, 3, 3, 3])
    y0 = st(*ptrs, xc, efc, mn, me)[1].clone()
    assert st.on_tables
    other = make_layer("source_to_target", seed=6).state_dict()

    def packs_now():
        return CountLayerStep(plan, layer, [3, 3, 3, 3], force_packs=True)(*ptrs, xc, efc, mn, me)[1]

    assert torch.equal(_bits(y0), _bits(packs_now()))
    with torch.no_grad():
        layer.msg_fn.fc[0].weight[:, :28].mul_(-1.5)              # the x_i columns and nothing else
    y1 = st(*ptrs, xc, efc, mn, me)[1].clone()
    assert not torch.equal(y1, y0) and torch.equal(_bits(y1), _bits(packs_now()))
    with torch.no_grad():
        layer.msg_fn.fc[0].bias.add_(0.25)                        # the folded bias (column 31 of the x_i chunks)
    y2 = st(*ptrs, xc, efc, mn, me)[1].clone()
    assert not torch.equal(y2, y1) and torch.equal(_bits(y2), _bits(packs_now()))
    layer.load_state_dict(other)
    y3 = st(*ptrs, xc, efc, mn, me)[1].clone()
    assert not torch.equal(y3, y2) and torch.equal(_bits(y3), _bits(packs_now()))


@no_cache
def test_tables_under_capture_and_replay():
    """GraphedStep over the step: the replayed rows equal the eager ones, also after the codes were refilled"""
    from gsn_amd import layers
    from gsn_amd.counting import CountPlan
    from gsn_amd.graphs import GraphedStep
    from gsn_amd.step import CountLayerStep
    b, ptrs, atoms, bonds = _zinc(64, 84)
    mn, me = _sizes(b)
    plan = CountPlan.get(cycles(), "edge", False)
    layer = make_layer("source_to_target", seed=2)
    xc, efc = layers.Codes(atoms, [28]), layers.Codes(bonds, [4])
    eager = CountLayerStep(plan, layer, [3, 3, 3, 3])
    ids0, y0, _ = eager(*ptrs, xc, efc, mn, me)
    ids0, y0 = ids0.clone(), y0.clone()
    step = CountLayerStep(plan, layer, [3, 3, 3, 3])
    g = GraphedStep(lambda: step(*ptrs, xc, efc, mn, me))
    ids_g, y_g, _ = g()
    torch.cuda.synchronize()
    assert step.on_tables and torch.equal(ids_g, ids0) and torch.equal(_bits(y_g), _bits(y0))
    atoms.copy_((atoms + 3) % 28); bonds.copy_((bonds + 1) % 4)
    g()
    ids1, y1, _ = eager(*ptrs, xc, efc, mn, me)
    torch.cuda.synchronize()
    assert torch.equal(ids_g, ids1) and torch.equal(_bits(y_g), _bits(y1)) and not torch.equal(y1, y0)


def test_tables_against_float64(monkeypatch, capfd):
    """the seven-graph batch against the float64 layer by the check of tests/layer_ref.py (tests/test_layer_f64_gpu.py's tolerance: max and rms
    of |y - y64| / sigma within 4 x the fp32 oracle's); the pack path is put through the same check and must not pass where tables fail"""
    import layer_ref as R
    from gsn_amd import layers, synth
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    b, ptrs, atoms, bonds = _zinc(7, 85)
    mn, me = _sizes(b)
    cls = "GSN_edge_sparse"
    ctor = dict(d_in=28, d_ef=4, d_id=12, id_scope="local", d_degree=1, degree_as_tag=False, retain_features=True, seed=0, activation_name="relu",
                bn=True, msg_kind="general", flow="source_to_target", d_msg=128, d_up=128, d_h=[128])
    layer, sd = R.layer_state(cls, ctor, 31)
    layer.to(_dev())
    plan = CountPlan.get(cycles(), "edge", False)
    xc, efc = layers.Codes(atoms, [28]), layers.Codes(bonds, [4])
    st = CountLayerStep(plan, layer, [3, 3, 3, 3])
    ids, y_t, _ = st(*ptrs, xc, efc, mn, me)
    y_p = CountLayerStep(plan, layer, [3, 3, 3, 3], force_packs=True)(*ptrs, xc, efc, mn, me)[1]
    assert st.on_tables
    one_hot = torch.nn.functional.one_hot
    x, ef = one_hot(atoms.cpu(), 28).float(), one_hot(bonds.cpu(), 4).float()
    idf = one_hot(ids.cpu().clamp(max=2), 3).reshape(b.num_edges, 12).float()
    ei = torch.from_numpy(b.edge_index)
    y64, sigma = R.reference(cls, ctor, sd, x, ei, idf, ef)
    y32 = R.oracle32(cls, ctor, sd, x, ei, idf, ef)
    assert bool((sigma > 0).all())
    q32 = ((y32.double() - y64).abs() / sigma)
    for name, y in (("packs", y_p), ("tables", y_t)):
        q = ((y.cpu().double() - y64).abs() / sigma)
        print("%s: max q %.3f (fp32 oracle %.3f)  rms q %.3f (fp32 oracle %.3f)" % (name, float(q.max()), float(q32.max()), float(q.pow(2).mean().sqrt()),
                                                                                  float(q32.pow(2).mean().sqrt())))
        assert float(q32.max()) <= 32 and float(q32.pow(2).mean().sqrt()) <= 4
        assert float(q.max()) <= 4 * float(q32.max()) and float(q.pow(2).mean().sqrt()) <= 4 * float(q32.pow(2).mean().sqrt()), name
