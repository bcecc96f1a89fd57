"""The tile loop of the packed-row layer kernel (csrc/layer_rp.hip) on the tile shapes at which its block loop can go wrong: the tile's first
block peeled out of the loop and started from a zero C operand, the per-node sums accumulated in place over the further blocks, two gather
sets taking turns, tiles without any edge, waves that walk several tiles.

Every case runs layer 0 three ways -- ``CountLayerStep`` on code keys, ``CountLayerStep(force_packs=True)`` on row packs, and the layer's
own forward on ``Codes`` inputs -- and asserts

* the three results equal bit for bit,
* within the element-wise bound of tests/test_pack16_gpu.py (1e-5 relative + 1e-5 of the row maximum) of ``oracle.layer_forward``,
* equal, bit for bit, to rows recorded from the library of the commit BEFORE the loop was restructured
  (tests/golden/layer_rp_parent_rows.npz: a fixed sample of rows per case).  The restructuring removed register copies, a zero fill and
  scalar address set-up; it changed no arithmetic, and this is what holds it to that.

The recorded rows were written by this file itself, run as a script against the earlier build of the same ABI:

    GSN_LIB_PATH=<earlier build>/libgsn_hip.so python tests/test_layer_rp_tiles_gpu.py tests/golden/layer_rp_parent_rows.npz [case ...]
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_rp_parent_rows.npz")
ID_CLASSES = [3, 3, 3, 3]
# a launch of fewer workgroups than this splits a heavy graph (>= 1024 cells) over several of them, which the step's side workgroups do not
# ride (csrc/count.hip): the cases with one heavy graph carry this many molecules behind it
N_PAD = 2048


def _star(n_leaves, repeats):
    """A hub (vertex 0) whose ``n_leaves`` leaves are each named ``repeats`` times, both directions: in-degree n_leaves * repeats."""
    leaves = np.tile(np.arange(1, n_leaves + 1, dtype=np.int64), repeats)
    hub = np.zeros_like(leaves)
    return n_leaves + 1, np.concatenate([np.stack([leaves, hub]), np.stack([hub, leaves])], axis=1)


def _graphs(case):
    from gsn_amd import synth
    rng = np.random.default_rng(2024)
    empty = np.zeros((2, 0), dtype=np.int64)
    mol = lambda k: [synth.zinc_shape_graph(rng) for _ in range(k)]
    if case in ("a_three_molecules", "f_identity_no_bn"):
        return mol(3)
    if case == "b_dense_tile":                 # 40 vertices, 300 columns: ~7.5 in-edges per vertex, a tile of 32 vertices has ~8 blocks
        return [synth.er_graph(40, 150, 7)] + mol(N_PAD)
    if case == "c_edgeless_tiles":             # ~100 nodes = 4 wave ranges of one tile each: tiles without any column, a tile that starts edge-less, the batch's end
        return [(70, empty)] + mol(1) + [(5, empty)]
    if case == "g_edgeless_tile_then_tile":    # ranges of two tiles, as in e, with a run of 70 edge-less vertices behind every 100th molecule: some
        m = mol(3000)                          # range starts in a run and leaves it in its second tile -- a tile without edges (the zero-fill arm)
        out = []                               # IN FRONT of a tile with edges (a peeled block) in the same wave
        for i in range(0, 3000, 100):
            out += m[i:i + 100] + [(70, empty)]
        return out
    if case == "d_star_3000":                  # one target across 94 blocks (the counting kernel takes <= 768 vertices: 100 leaves named 30 times)
        return [_star(100, 30)] + mol(N_PAD)
    if case == "e_two_tiles_per_wave":
        return mol(3000)
    raise KeyError(case)


CASES = ["a_three_molecules", "b_dense_tile", "c_edgeless_tiles", "d_star_3000", "e_two_tiles_per_wave", "f_identity_no_bn", "g_edgeless_tile_then_tile"]


def _ctor(case):
    ident = case == "f_identity_no_bn"
    return dict(d_in=28, d_ef=4, d_id=12, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128, d_up=128,
                d_h=[128], seed=0, activation_name="identity" if ident else "relu", bn=not ident, msg_kind="general", flow="source_to_target")


def _sample_rows(n, deg=None, case=""):
    """The recorded rows of a case: its first 64 (the hand-made graph leads the batch), its last 16, 16 in between; case g: the last rows of every edge-less
    run and the nine behind it (where a wave's second tile leaves the run)."""
    if n <= 96:
        return np.arange(n)
    if case == "g_edgeless_tile_then_tile":
        zero = np.flatnonzero(deg == 0)
        runs = [r for r in np.split(zero, np.flatnonzero(np.diff(zero) != 1) + 1) if len(r) >= 40]
        return np.unique(np.concatenate([np.arange(max(r[-1] - 3, 0), min(r[-1] + 10, n)) for r in runs]))
    mid = np.random.default_rng(n).integers(64, n - 16, 16)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(n - 16, n)]))


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_case(case):
    """-> (y on keys, y on packs, y of layer(Codes), oracle rows) of one case, the first three on the GPU."""
    import networkx as nx
    from gsn_amd import layers, synth
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    from oracle import oracle
    dev = torch.device("cuda", 0)
    b = synth.collate(_graphs(case))
    N, E = b.num_nodes, b.num_edges
    rng = np.random.default_rng(len(case) + N)
    atoms_h, bonds_h = rng.integers(0, 28, N), rng.integers(0, 4, E)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    node_ptr, edge_ptr, ei, atoms, bonds = t(b.node_ptr), t(b.edge_ptr), t(b.edge_index), t(atoms_h), t(bonds_h)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    ctor = _ctor(case)
    torch.manual_seed(11)
    layer = layers.GSN_edge_sparse(**ctor).eval()
    with torch.no_grad():                       # running statistics that are not the identity
        for m in layer.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    layer.to(dev)
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    ys = []
    for force in (False, True):
        step = CountLayerStep(plan, layer, ID_CLASSES, clamp=True, force_packs=force)
        ids, y, _ = step(node_ptr, edge_ptr, ei, layers.Codes(atoms, [28]), layers.Codes(bonds, [4]), mn, me)
        torch.cuda.synchronize()
        assert step.on_keys == (not force)
        step.check_status()
        ys.append(y)
    with torch.no_grad():
        y3 = layer(layers.Codes(atoms, [28]), ei, identifiers=layers.Codes(ids, ID_CLASSES, clamp=True), degrees=torch.zeros(N, device=dev),
                   edge_features=layers.Codes(bonds, [4]))
    torch.cuda.synchronize()
    x = torch.nn.functional.one_hot(torch.from_numpy(atoms_h), 28).float()
    ef = torch.nn.functional.one_hot(torch.from_numpy(bonds_h), 4).float()
    idf = torch.nn.functional.one_hot(ids.cpu().clamp(max=2), 3).reshape(E, 12).float()
    ref = oracle.layer_forward("GSN_edge_sparse", ctor, sd, x, torch.from_numpy(b.edge_index), identifiers=idf, degrees=None, edge_features=ef,
                               training=False)
    deg = np.bincount(b.edge_index[1], minlength=N)
    return ys[0], ys[1], y3, ref, deg


def _tile_shape_holds(case, deg):
    """The property of the batch that makes it the case it is meant to be."""
    if case == "b_dense_tile":
        return deg[:32].sum() >= 5 * 32                       # the first tile: five or more blocks of 32 rows
    if case == "c_edgeless_tiles":
        return deg[:70].sum() == 0 and deg[-5:].sum() == 0 and deg.sum() > 0
    if case == "d_star_3000":
        return deg[0] == 3000
    if case == "e_two_tiles_per_wave":
        return len(deg) > 33 * 2048                           # 2 048 wave ranges of more than 32 nodes each: two tiles or more
    if case == "g_edgeless_tile_then_tile":
        # the launcher's ranges (csrc/layer_rp.hip: 2 048 of them, the first 60 % of the nodes to the older half of the waves): at least two of
        # them have a first tile of 32 nodes without any in-edge and in-edges behind it
        n, half = len(deg), 1024
        n_split = int(n * 0.6)
        hits = 0
        for base, cnt in ((0, n_split), (n_split, n - n_split)):
            for i in range(half):
                lo, hi = base + cnt * i // half, base + cnt * (i + 1) // half
                hits += hi - lo > 32 and deg[lo:lo + 32].sum() == 0 and deg[lo + 32:hi].sum() > 0
        return n >= 32 * 2048 and hits >= 2
    return len(deg) <= 3 * 38


@pytest.fixture(scope="module")
def parent_rows():
    with np.load(GOLDEN_FILE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES)
def test_tile_loop_rows_equal_on_all_paths_and_to_the_parent(case, parent_rows):
    y_keys, y_packs, y_layer, ref, deg = run_case(case)
    assert _tile_shape_holds(case, deg)
    assert torch.equal(_bits(y_keys), _bits(y_packs))
    assert torch.equal(_bits(y_keys), _bits(y_layer))
    got = y_keys.cpu()
    floor = 1e-5 * ref.abs().amax(dim=1, keepdim=True)
    excess = ((got - ref).abs() - (1e-5 * ref.abs() + floor)).max().item()
    print("%s: N %d, largest |y - oracle| / max|oracle| %.3g, excess over the bound %.3g" % (case, got.shape[0], float((got - ref).abs().max() / ref.abs().max()), excess))
    assert bool(((got - ref).abs() <= 1e-5 * ref.abs() + floor).all())
    rows = _sample_rows(got.shape[0], deg, case)
    assert np.array_equal(parent_rows[case + "_rows"], rows)
    assert np.array_equal(got[rows].numpy().view(np.int32), parent_rows[case].view(np.int32))


if __name__ == "__main__":          # record the sample rows with the library in use (GSN_LIB_PATH): see the module's docstring
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    if os.path.exists(sys.argv[1]):            # (cases named behind the file are recorded into it, the others kept)
        with np.load(sys.argv[1]) as z:
            out = {k: z[k] for k in z.files}
    for case in (sys.argv[2:] or CASES):
        y_keys, y_packs, y_layer, ref, deg = run_case(case)
        assert _tile_shape_holds(case, deg), case
        assert torch.equal(_bits(y_keys), _bits(y_packs)) and torch.equal(_bits(y_keys), _bits(y_layer)), case
        rows = _sample_rows(y_keys.shape[0], deg, case)
        out[case] = y_keys.cpu().numpy()[rows]
        out[case + "_rows"] = rows
        print("%s: N %d, %d rows, |y - oracle| / max %.3g" % (case, y_keys.shape[0], len(rows), float((y_keys.cpu() - ref).abs().max() / ref.abs().max())), flush=True)
    np.savez_compressed(sys.argv[1], **out)
