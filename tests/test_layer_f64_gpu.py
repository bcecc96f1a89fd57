"""Every one-launch `general` layer kernel against a float64 evaluation of the same layer, element by element, on batches whose in-degrees
sit at the tile iterators' boundaries (tests/layer_ref.py: 0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, a hub of 300, runs of isolated
nodes; the same list behind 1 and 31 leading nodes; four copies of it), with the launcher's own grid and with ``GSN_FUSED_GRID`` = 1 and 3
(the switch is read at every launch: a 257-node batch then has the many-tiles-per-wave shape that otherwise takes 65 000 nodes).

Every case
  * runs the layer in eval mode under ``GSN_CHAIN_TRACE`` and asserts that the trace names the kernel (and instantiation) it is meant for,
    and -- from the trace's ``grid`` / ``ranges`` fields -- that the small grid was taken;
  * applies the check of tests/layer_ref.py to ALL output elements: q = |y - y64| / sigma, max q <= 4 max q32 and rms q <= 4 rms q32,
    q32 being the same quotient of the fp32 oracle on the same case, inside its caps (max q32 <= 32, rms q32 <= 4, sigma > 0);
  * asserts that no output element is non-finite.

Kernels by case id: ``rr`` layer_fused_kernel_rr<4,2>; ``rp`` layer_fused_kernel_rp<4,2> on row packs and on Codes; ``keys``
layer_fused_kernel_rp<4,2> keys (through CountLayerStep); ``f10_8_4`` layer_fused_kernel<5,10,8,4>; ``f6_4_2`` <5,6,4,2>; ``g6_4`` /
``g6_8`` / ``g10_4`` / ``g10_8`` the generic <5,6,4,0>, <5,6,8,0>, <5,10,4,0>, <5,10,8,0>; ``w`` layer_fused_kernel_w; ``g``
layer_fused_kernel_g (and its fall-back to w on a 129-vertex graph); ``multi`` the multi-launch path (chain + propagate kernels).

The layer classes give msg_fn and update_fn one ``d_h``, so edge and node0 stage have one width; <5,6,8,0> (k0 = d_x + n_edge + 4 <= 96
with k1 = n_node0 > 64) and the 96 / 64 / 128 example of <5,10,4,0> need two, and get an update_fn with a hidden width of its own
(layer_ref.layer_state(d_h_up=...)).

Largest share of the factor 4 seen per kernel on an MI355X (max q / max q32, rms q / rms q32; printed by the last test of the module):

    kernel                                  max q / max q32    rms q / rms q32    cases
    layer_fused_kernel_rr<4,2>              1.35               1.14               69
    layer_fused_kernel_rp<4,2>              1.21               1.20               50
    layer_fused_kernel_rp<4,2> keys         1.07               1.24                3
    layer_fused_kernel<5,10,8,4>            0.83               0.84               13
    layer_fused_kernel<5,6,4,2>             1.10               0.94               13
    layer_fused_kernel<5,6,4,0>             1.04               1.03               12
    layer_fused_kernel<5,6,8,0>             0.86               0.95               12
    layer_fused_kernel<5,10,4,0>            0.98               0.91               12
    layer_fused_kernel<5,10,8,0>            0.95               0.93               12
    layer_fused_kernel_w                    1.15               1.23               42
    layer_fused_kernel_g                    1.16               1.08               33
    multi-launch path                       1.41               1.54                5

No kernel is above 2, i.e. none uses more than about a third of the factor; the multi-launch path (bf16x6 chain kernels) and rr come
closest.  No case failed, so no kernel finding came out of this module.
"""
import re

import numpy as np
import pytest
import torch

import layer_ref as R

pytestmark = pytest.mark.gpu

GRIDS = [None, 1, 3]

RR = "layer_fused_kernel_rr<4,2> nodes"
RP = "layer_fused_kernel_rp<4,2> nodes"
RPK = "layer_fused_kernel_rp<4,2> keys nodes"
KW = "layer_fused_kernel_w nodes"
KG = "layer_fused_kernel_g nodes"
LF = lambda a, b, c, d: "layer_fused_kernel<%d,%d,%d,%d> nodes" % (a, b, c, d)

_SEEN = {}          # kernel -> [largest max-ratio, largest rms-ratio, cases]


def _ctor(**over):
    base = dict(d_degree=1, degree_as_tag=False, retain_features=True, seed=0, activation_name="relu", bn=True, msg_kind="general",
                flow="source_to_target", d_msg=128, d_up=128, d_h=[128])
    base.update(over)
    return base


GSN_E = ("GSN_edge_sparse", _ctor(d_in=28, d_ef=4, d_id=12, id_scope="local"), 28, 12, 4)
GSN_E4 = ("GSN_edge_sparse", _ctor(d_in=4, d_ef=4, d_id=12, id_scope="local"), 4, 12, 4)
GSN_V = ("GSN_sparse", _ctor(d_in=16, d_id=8, id_scope="global"), 16, 8, 0)
GSN_L = ("GSN_sparse", _ctor(d_in=28, d_id=16, id_scope="local"), 28, 16, 0)
MPNN_E = ("MPNN_edge_sparse", _ctor(d_in=28, d_ef=4), 28, 0, 4)
MPNN28 = ("MPNN_sparse", _ctor(d_in=28), 28, 0, 0)
MPNN4 = ("MPNN_sparse", _ctor(d_in=4), 4, 0, 0)


def _with(spec, **over):
    return (spec[0], dict(spec[1], **over)) + tuple(spec[2:])


_REFS = {}


def _case(spec, kind, lead=0, repeat=1, per_graph=None, d_h_up=None, seed=11):
    """the case's layer parameters, inputs, float64 reference, rounding scale and fp32 oracle: computed once on the CPU, shared by the grid
    parameters and left unchanged"""
    cls, ctor, d_x, d_id, d_ef = spec
    key = (cls, tuple(sorted((k, str(v)) for k, v in ctor.items())), kind, lead, repeat, str(per_graph), str(d_h_up), seed)
    if key not in _REFS:
        n, ei, node_ptr = R.boundary_batch(seed, per_graph=per_graph, lead=lead, repeat=repeat)
        if ctor.get("flow") == "target_to_source":
            ei = ei.flip(0).contiguous()                  # (the prescribed in-degrees belong to the aggregating end)
        _, sd = R.layer_state(cls, ctor, seed + 1, d_h_up=d_h_up)
        x, ids, ef = R.make_inputs(kind, seed + 2, n, ei.shape[1], d_x, d_id, d_ef, ids_per_node=ctor.get("id_scope") == "global")
        y64, sigma = R.reference(cls, ctor, sd, x, ei, ids, ef)
        y32 = R.oracle32(cls, ctor, sd, x, ei, ids, ef)
        R.yardstick(y32, y64, sigma)
        _REFS[key] = dict(cls=cls, ctor=ctor, sd=sd, x=x, ei=ei, ids=ids, ef=ef, y64=y64, sigma=sigma, y32=y32, n=n, node_ptr=node_ptr,
                          d_h_up=d_h_up, seed=seed)
    return _REFS[key]


def _layer(c):
    layer, _ = R.layer_state(c["cls"], c["ctor"], c["seed"] + 1, d_h_up=c["d_h_up"])
    layer.load_state_dict(c["sd"])
    return layer.cuda().eval()


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("GSN_FUSED_GRID", raising=False)
    else:
        monkeypatch.setenv("GSN_FUSED_GRID", str(grid))


def _traced(monkeypatch, capfd, fn):
    """-> (result, the launch trace on stderr)"""
    from gsn_amd import layers
    layers._CSR_CACHE.clear()
    capfd.readouterr()
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")
    try:
        try:
            with torch.no_grad():
                y = fn()
            torch.cuda.synchronize()
        except RuntimeError as e:            # a GPU error ends the run: nothing more is launched on a device that has faulted
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                pytest.exit("GPU error, no further launches: %s" % e, returncode=3)
            raise
    finally:
        monkeypatch.delenv("GSN_CHAIN_TRACE")
    return y, capfd.readouterr().err


def _forward(c, monkeypatch, capfd, grid, prepare=None, inputs=None, partition=False):
    """the layer of case ``c`` on the GPU under the trace; ``prepare(x, ids, ef)``: tags the device tensors (row packs); ``inputs``: other
    device inputs that stand for the same values (Codes); ``partition``: registers the graph boundaries"""
    from gsn_amd import layers
    layer = _layer(c)
    dev = torch.device("cuda", 0)
    g = lambda t: None if t is None else t.to(dev)
    x, ids, ef = inputs if inputs is not None else (g(c["x"]), g(c["ids"]), g(c["ef"]))
    eig = c["ei"].to(dev)
    if partition:
        eptr = R.edge_ptr_of(c["ei"], c["node_ptr"])
        mn, me = int((c["node_ptr"][1:] - c["node_ptr"][:-1]).max()), int((eptr[1:] - eptr[:-1]).max())
        assert layers.set_graph_partition(eig, c["node_ptr"].to(dev), eptr.to(dev), mn, me)
    if prepare is not None:
        prepare(x, ids, ef)
    kw = dict(identifiers=ids, degrees=torch.zeros(c["n"], device=dev))
    if ef is not None:
        kw["edge_features"] = ef
    _set_grid(monkeypatch, grid)
    y, trace = _traced(monkeypatch, capfd, lambda: layer(x, eig, **kw))
    return y.cpu(), trace


def _line(trace, kernel):
    hits = [ln for ln in trace.splitlines() if kernel in ln]
    assert len(hits) == 1, "expected one launch of %r, trace:\n%s" % (kernel, trace[-1500:])
    return hits[0]


def _assert_grid(line, grid, n, tiles_per_range=None):
    """the launcher's own report: the forced grid was taken (and, where it prints its wave ranges, how many tiles a range holds)"""
    got = int(re.search(r"grid (\d+)", line).group(1))
    m = re.search(r"ranges (\d+)", line)
    if grid is None:
        assert got > 3, line
    else:
        assert got == grid, line
        if m is not None:
            assert int(m.group(1)) <= 8 * grid, line
    if tiles_per_range is not None:
        assert m is not None and n >= 32 * tiles_per_range * int(m.group(1)), line


def _check(c, y, kernel, what, factor=R.FACTOR):
    assert y.shape == c["y64"].shape and bool(torch.isfinite(y).all()), what
    r = R.check(y, c["y32"], c["y64"], c["sigma"], factor=factor, what=what)
    s = _SEEN.setdefault(kernel, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], r[0]), max(s[1], r[1]), s[2] + 1
    print("%s [%s]: max q / max q32 %.2f, rms q / rms q32 %.2f" % (what, kernel, r[0], r[1]))
    return r


# ------------------------------------------------------------------------------------------------------------------------------------
# layer_fused_kernel_rr<4,2>: every stage 128 wide, d_x + 4 <= 32, untagged float inputs
# ------------------------------------------------------------------------------------------------------------------------------------
RR_CASES = {
    "gsn_e-exact": (GSN_E, "exact", {}),
    "gsn_e-real": (GSN_E, "real", {}),
    "gsn_e-mixed": (GSN_E, "mixed", {}),
    "gsn_e-exact-lead1": (GSN_E, "exact", dict(lead=1)),
    "gsn_e-real-lead31": (GSN_E, "real", dict(lead=31)),
    "gsn_e-mixed-lead31": (GSN_E, "mixed", dict(lead=31)),
    "gsn_e-exact-t2s": (_with(GSN_E, flow="target_to_source"), "exact", {}),
    "gsn_e-real-t2s-lead1": (_with(GSN_E, flow="target_to_source"), "real", dict(lead=1)),
    "gsn_e-real-identity-bn": (_with(GSN_E, activation_name="identity"), "real", {}),
    "gsn_e-exact-identity-bn": (_with(GSN_E, activation_name="identity"), "exact", {}),
    "gsn_e-exact-relu-nobn": (_with(GSN_E, bn=False), "exact", {}),
    "gsn_e-real-relu-nobn": (_with(GSN_E, bn=False), "real", dict(lead=31)),
    "gsn_e-d4-exact": (GSN_E4, "exact", {}),
    "gsn_e-d4-real": (GSN_E4, "real", dict(lead=1)),
    "gsn_v-global-real": (GSN_V, "real", {}),
    "gsn_v-global-exact": (GSN_V, "exact", dict(lead=31)),
    "mpnn-d28-real": (MPNN28, "real", {}),
    "mpnn-d4-exact": (MPNN4, "exact", {}),
    "mpnn-d4-real": (MPNN4, "real", dict(lead=31)),
    "mpnn_e-real": (MPNN_E, "real", dict(lead=1)),
}


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("name", sorted(RR_CASES))
def test_rr(name, grid, monkeypatch, capfd):
    spec, kind, kw = RR_CASES[name]
    c = _case(spec, kind, **kw)
    y, trace = _forward(c, monkeypatch, capfd, grid)
    _assert_grid(_line(trace, RR), grid, c["n"])
    _check(c, y, RR, "rr %s grid %s" % (name, grid))


@pytest.mark.parametrize("grid", [1, 3], ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("kind", ["exact", "real", "mixed"])
def test_rr_many_tiles_per_wave(kind, grid, monkeypatch, capfd):
    """1 028 nodes (the degree list four times): with one workgroup every wave range holds four tiles or more"""
    c = _case(GSN_E, kind, repeat=4)
    y, trace = _forward(c, monkeypatch, capfd, grid)
    _assert_grid(_line(trace, RR), grid, c["n"], tiles_per_range=4 if grid == 1 else 1)
    _check(c, y, RR, "rr x4 %s grid %s" % (kind, grid))


# ------------------------------------------------------------------------------------------------------------------------------------
# layer_fused_kernel_rp<4,2>: the same shapes on tagged row packs and on Codes inputs (exact inputs only)
# ------------------------------------------------------------------------------------------------------------------------------------
def _tag(x, ids, ef):
    from gsn_amd import packs
    packs.node_pack(x)
    per_edge = [t for t in (ids, ef) if t is not None]
    if per_edge:
        packs.edge_pack(per_edge)


RP_CASES = {
    "gsn_e-pack": (GSN_E, "pack", {}),
    "gsn_e-binary": (GSN_E, "binary", {}),
    "gsn_e-pack-lead1": (GSN_E, "pack", dict(lead=1)),
    "gsn_e-pack-lead31": (GSN_E, "pack", dict(lead=31)),
    "gsn_e-pack-t2s": (_with(GSN_E, flow="target_to_source"), "pack", {}),
    "gsn_e-pack-identity-bn": (_with(GSN_E, activation_name="identity"), "pack", {}),
    "gsn_e-pack-relu-nobn": (_with(GSN_E, bn=False), "pack", dict(lead=31)),
    "gsn_e-d4-pack": (GSN_E4, "pack", {}),
    "gsn_l-pack": (GSN_L, "pack", dict(lead=1)),
    "mpnn-d28-pack": (MPNN28, "pack", {}),
    "mpnn-d4-pack": (MPNN4, "pack", dict(lead=31)),
    "mpnn_e-pack": (MPNN_E, "pack", {}),
}


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("name", sorted(RP_CASES))
def test_rp_row_packs(name, grid, monkeypatch, capfd):
    spec, kind, kw = RP_CASES[name]
    c = _case(spec, kind, **kw)
    y, trace = _forward(c, monkeypatch, capfd, grid, prepare=_tag)
    _assert_grid(_line(trace, RP), grid, c["n"])
    _check(c, y, RP, "rp %s grid %s" % (name, grid))


@pytest.mark.parametrize("grid", [1, 3], ids=lambda g: "grid-%s" % g)
def test_rp_many_tiles_per_wave(grid, monkeypatch, capfd):
    c = _case(GSN_E, "pack", repeat=4)
    y, trace = _forward(c, monkeypatch, capfd, grid, prepare=_tag)
    _assert_grid(_line(trace, RP), grid, c["n"], tiles_per_range=4 if grid == 1 else 1)
    _check(c, y, RP, "rp x4 pack grid %s" % grid)


ID_CLASSES = [3, 3, 3, 3]


def _codes_case(lead, repeat, flow):
    """GSN_edge_sparse 28 / 12 / 4 on integer codes: the float64 reference takes their one-hot rows"""
    spec = _with(GSN_E, flow=flow)
    key = ("codes", lead, repeat, flow)
    if key not in _REFS:
        n, ei, node_ptr = R.boundary_batch(13, lead=lead, repeat=repeat)
        if flow == "target_to_source":
            ei = ei.flip(0).contiguous()
        E = ei.shape[1]
        g = torch.Generator().manual_seed(17)
        atoms, bonds = torch.randint(0, 28, (n,), generator=g), torch.randint(0, 4, (E,), generator=g)
        idc = torch.randint(0, 3, (E, 4), generator=g)
        one_hot = torch.nn.functional.one_hot
        x, ef, ids = one_hot(atoms, 28).float(), one_hot(bonds, 4).float(), one_hot(idc, 3).reshape(E, 12).float()
        _, sd = R.layer_state(spec[0], spec[1], 14)
        y64, sigma = R.reference(spec[0], spec[1], sd, x, ei, ids, ef)
        y32 = R.oracle32(spec[0], spec[1], sd, x, ei, ids, ef)
        R.yardstick(y32, y64, sigma)
        _REFS[key] = dict(cls=spec[0], ctor=spec[1], sd=sd, x=x, ei=ei, ids=ids, ef=ef, y64=y64, sigma=sigma, y32=y32, n=n, node_ptr=node_ptr,
                          d_h_up=None, seed=13, codes=(atoms, idc, bonds))
    return _REFS[key]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("lead,repeat,flow", [(0, 1, "source_to_target"), (31, 1, "source_to_target"), (1, 1, "target_to_source"), (0, 4, "source_to_target")])
def test_rp_codes(lead, repeat, flow, grid, monkeypatch, capfd):
    from gsn_amd import layers
    c = _codes_case(lead, repeat, flow)
    atoms, idc, bonds = (t.cuda() for t in c["codes"])
    inputs = (layers.Codes(atoms, [28]), layers.Codes(idc, ID_CLASSES, clamp=True), layers.Codes(bonds, [4]))
    y, trace = _forward(c, monkeypatch, capfd, grid, inputs=inputs)
    _assert_grid(_line(trace, RP), grid, c["n"], tiles_per_range=4 if (repeat == 4 and grid == 1) else None)
    _check(c, y, RP, "rp codes lead %d x%d %s grid %s" % (lead, repeat, flow, grid))


# ------------------------------------------------------------------------------------------------------------------------------------
# layer_fused_kernel: <5,10,8,4> (all widths 128 where rr refuses: K_e = 80), <5,6,4,2> (all widths 64), the four generic instantiations
# ------------------------------------------------------------------------------------------------------------------------------------
GSN_E80 = ("GSN_edge_sparse", _ctor(d_in=28, d_ef=4, d_id=20, id_scope="local"), 28, 20, 4)
GSN_E64 = ("GSN_edge_sparse", _ctor(d_in=28, d_ef=4, d_id=12, id_scope="local", d_msg=64, d_up=64, d_h=[64]), 28, 12, 4)
W = lambda d_h, d_msg, d_up: ("GSN_edge_sparse", _ctor(d_in=28, d_ef=4, d_id=12, id_scope="local", d_msg=d_msg, d_up=d_up, d_h=[d_h]), 28, 12, 4)

# id -> (kernel, spec, update_fn's own hidden width or None): stage widths edge / node0 / node1, k0 = 28 + edge + 4, k1 = node0
LF_SHAPES = {
    "f10_8_4": (LF(5, 10, 8, 4), GSN_E80, None),                      # 128 / 128 / 128, K_e = 80
    "f6_4_2": (LF(5, 6, 4, 2), GSN_E64, None),                        # 64 / 64 / 64
    "g6_4": (LF(5, 6, 4, 0), W(32, 96, 96), None),                    # 32 / 32 / 96:  k0 = 64,  k1 = 32
    "g6_8": (LF(5, 6, 8, 0), W(32, 64, 64), [96]),                    # 32 / 96 / 64:  k0 = 64,  k1 = 96
    "g10_4": (LF(5, 10, 4, 0), W(96, 64, 128), [64]),                 # 96 / 64 / 128: k0 = 128, k1 = 64
    "g10_8": (LF(5, 10, 8, 0), W(96, 128, 128), None),                # 96 / 96 / 128: k0 = 128, k1 = 96
}


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("kind,lead", [("exact", 0), ("real", 0), ("mixed", 31), ("real", 1)])
@pytest.mark.parametrize("shape", sorted(LF_SHAPES))
def test_layer_fused_instantiations(shape, kind, lead, grid, monkeypatch, capfd):
    kernel, spec, d_h_up = LF_SHAPES[shape]
    c = _case(spec, kind, lead=lead, d_h_up=d_h_up)
    y, trace = _forward(c, monkeypatch, capfd, grid)
    _assert_grid(_line(trace, kernel), grid, c["n"])
    _check(c, y, kernel, "%s %s lead %d grid %s" % (shape, kind, lead, grid))


@pytest.mark.parametrize("shape", ["f10_8_4", "f6_4_2"])
def test_layer_fused_many_tiles_per_workgroup(shape, monkeypatch, capfd):
    kernel, spec, d_h_up = LF_SHAPES[shape]
    c = _case(spec, "real", repeat=4, d_h_up=d_h_up)
    y, trace = _forward(c, monkeypatch, capfd, 1)
    _assert_grid(_line(trace, kernel), 1, c["n"])
    _check(c, y, kernel, "%s x4 real grid 1" % shape)


# ------------------------------------------------------------------------------------------------------------------------------------
# layer_fused_kernel_w / layer_fused_kernel_g: d_x = 128, the five rows of WIDE in tests/test_fused_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------------
WIDE = {
    "gsn_e": ("GSN_edge_sparse", _ctor(d_in=128, d_ef=4, d_id=12, id_scope="local"), 128, 12, 4),
    "mpnn_e": ("MPNN_edge_sparse", _ctor(d_in=128, d_ef=4), 128, 0, 4),
    "gsn_l": ("GSN_sparse", _ctor(d_in=128, d_id=8, id_scope="local"), 128, 8, 0),
    "mpnn": ("MPNN_sparse", _ctor(d_in=128), 128, 0, 0),
    "gsn_v": ("GSN_sparse", _ctor(d_in=128, d_id=8, id_scope="global"), 128, 8, 0),
}


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("kind,lead", [("relu", 0), ("pow2", 31)])
@pytest.mark.parametrize("row", sorted(WIDE))
def test_w(row, kind, lead, grid, monkeypatch, capfd):
    c = _case(WIDE[row], kind, lead=lead)
    y, trace = _forward(c, monkeypatch, capfd, grid)
    _assert_grid(_line(trace, KW), grid, c["n"])
    _check(c, y, KW, "w %s %s grid %s" % (row, kind, grid))


@pytest.mark.parametrize("grid", [1, 3], ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("spec,kind", [(WIDE["gsn_e"], "pow2"), (_with(WIDE["gsn_e"], flow="target_to_source", activation_name="identity"), "relu"),
                                       (_with(WIDE["mpnn_e"], bn=False), "relu")], ids=["gsn_e-pow2", "gsn_e-t2s-identity-relu", "mpnn_e-nobn-relu"])
def test_w_many_tiles_per_wave(spec, kind, grid, monkeypatch, capfd):
    c = _case(spec, kind, repeat=4)
    y, trace = _forward(c, monkeypatch, capfd, grid)
    _assert_grid(_line(trace, KW), grid, c["n"], tiles_per_range=4 if grid == 1 else 1)
    _check(c, y, KW, "w x4 %s grid %s" % (kind, grid))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("kind", ["relu", "pow2"])
@pytest.mark.parametrize("row", sorted(WIDE))
def test_g(row, kind, grid, monkeypatch, capfd):
    """graphs of 1, 2, 127, 128, 128 and 5 vertices with registered boundaries, in-degrees up to 129 through repeated edges, a graph
    without any edge: csrc/layer_g.hip"""
    c = _case(WIDE[row], kind, per_graph=True)
    y, trace = _forward(c, monkeypatch, capfd, grid, partition=True)
    _assert_grid(_line(trace, KG), grid, c["n"])
    assert KW not in trace
    _check(c, y, KG, "g %s %s grid %s" % (row, kind, grid))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
def test_g_target_to_source_identity(grid, monkeypatch, capfd):
    c = _case(_with(WIDE["gsn_e"], flow="target_to_source", activation_name="identity"), "relu", per_graph=True)
    y, trace = _forward(c, monkeypatch, capfd, grid, partition=True)
    _assert_grid(_line(trace, KG), grid, c["n"])
    _check(c, y, KG, "g gsn_e t2s identity grid %s" % grid)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
def test_g_falls_back_to_w_on_a_129_vertex_graph(grid, monkeypatch, capfd):
    c = _case(WIDE["gsn_e"], "relu", per_graph=(1, 2, 127, 129, 128, 5))
    y, trace = _forward(c, monkeypatch, capfd, grid, partition=True)
    assert KG not in trace
    _assert_grid(_line(trace, KW), grid, c["n"])
    _check(c, y, KW, "g -> w on a 129-vertex graph grid %s" % grid)


# ------------------------------------------------------------------------------------------------------------------------------------
# the multi-launch path (flags.FUSED_LAYER = False: chain + propagate kernels), one case per class
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,kind", [(GSN_E, "real"), (GSN_V, "real"), (MPNN_E, "exact"), (MPNN28, "real"), (WIDE["gsn_e"], "relu")],
                         ids=["gsn_e", "gsn_v", "mpnn_e", "mpnn", "gsn_e-d128"])
def test_multi_launch_path(spec, kind, monkeypatch, capfd):
    from gsn_amd import flags
    monkeypatch.setattr(flags, "FUSED_LAYER", False)
    c = _case(spec, kind)
    y, trace = _forward(c, monkeypatch, capfd, None)
    assert "layer_fused_kernel" not in trace, trace[-800:]
    _check(c, y, "multi-launch", "multi-launch %s %s" % (spec[0], kind))


# ------------------------------------------------------------------------------------------------------------------------------------
# metamorphic: the nodes relabelled by a permutation (edge order, and with it every node's in-edge order, kept)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
@pytest.mark.parametrize("which", ["rr", "w"])
def test_relabelled_nodes_give_the_permuted_output(which, grid, monkeypatch, capfd):
    """y'[p[v]] of the relabelled batch against the float64 row of v, by the same check (equal bits are not required: the tiles differ)"""
    spec, kind, kernel = (GSN_V, "real", RR) if which == "rr" else (WIDE["gsn_v"], "pow2", KW)
    c = _case(spec, kind)
    n = c["n"]
    p = torch.from_numpy(np.random.default_rng(23).permutation(n))          # new label of node v
    inv = torch.empty_like(p)
    inv[p] = torch.arange(n)
    c2 = dict(c, x=c["x"][inv], ids=c["ids"][inv], ei=p[c["ei"]])           # (identifiers of the 'global' scope: one row per node)
    y2, trace = _forward(c2, monkeypatch, capfd, grid)
    _assert_grid(_line(trace, kernel), grid, n)
    _check(c, y2[p], kernel, "%s relabelled grid %s" % (which, grid))


# ------------------------------------------------------------------------------------------------------------------------------------
# layer_fused_kernel_rp<4,2> keys: through CountLayerStep
# ------------------------------------------------------------------------------------------------------------------------------------
def _boundary_graph():
    """One graph of <= 768 vertices that carries the boundary in-degrees, symmetric (the counting kernel takes undirected graphs), with
    repeated edges as the star of tests/test_layer_rp_tiles_gpu.py: hub h of in-degree d has ceil(d / 4) leaves of its own, named d times in
    all, both directions."""
    cols, n = [], 0
    for d in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300):
        n_leaves = (d + 3) // 4
        hub = n
        leaves = hub + 1 + (np.arange(d, dtype=np.int64) % n_leaves)
        hubs = np.full(d, hub, dtype=np.int64)
        cols += [np.stack([leaves, hubs]), np.stack([hubs, leaves])]
        n += 1 + n_leaves
    ei = np.concatenate(cols, axis=1)
    return n, ei[:, np.random.default_rng(3).permutation(ei.shape[1])]


N_PAD = 2048        # a counting launch of fewer workgroups splits a heavy graph over several of them, which the step's side workgroups do not ride


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "grid-%s" % g)
def test_rp_keys_through_the_count_layer_step(grid, monkeypatch, capfd):
    """One graph with hubs of in-degree 1, 31 .. 129 and 300 among ZINC-shaped molecules; the identifiers the step counts feed the float64
    reference.  The batch holds 2 048 molecules, not 40: below that many workgroups the counting launch splits the heavy graph and the
    step's entry point refuses the call (csrc/count.hip, as N_PAD of tests/test_layer_rp_tiles_gpu.py) -- the one case of this module
    beyond a few hundred nodes; its reference is computed once for the three grids.  csrc/layer_rp.hip's launcher reads GSN_FUSED_GRID
    for the keys variant too (rp_forward is one function)."""
    import networkx as nx
    from gsn_amd import layers, synth
    from gsn_amd.counting import CountPlan
    from gsn_amd.step import CountLayerStep
    rng = np.random.default_rng(2024)
    mols = [synth.zinc_shape_graph(rng) for _ in range(N_PAD)]
    b = synth.collate(mols[:20] + [_boundary_graph()] + mols[20:])
    N, E = b.num_nodes, b.num_edges
    deg = np.bincount(b.edge_index[1], minlength=N)
    assert {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300} <= set(deg.tolist()) and int(np.diff(b.node_ptr).max()) <= 768
    dev = torch.device("cuda", 0)
    rs = np.random.default_rng(N)
    atoms_h, bonds_h = rs.integers(0, 28, N), rs.integers(0, 4, E)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cls, ctor = GSN_E[0], GSN_E[1]
    layer, sd = R.layer_state(cls, ctor, 31)
    layer.to(dev)
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    step = CountLayerStep(plan, layer, ID_CLASSES, clamp=True)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    _set_grid(monkeypatch, grid)
    args = (t(b.node_ptr), t(b.edge_ptr), t(b.edge_index), layers.Codes(t(atoms_h), [28]), layers.Codes(t(bonds_h), [4]), mn, me)
    (ids, y, _), trace = _traced(monkeypatch, capfd, lambda: step(*args))
    assert step.on_keys
    step.check_status()
    _assert_grid(_line(trace, RPK), grid, N)
    ids = ids.cpu()
    if "keys" not in _REFS:
        one_hot = torch.nn.functional.one_hot
        x, ef = one_hot(torch.from_numpy(atoms_h), 28).float(), one_hot(torch.from_numpy(bonds_h), 4).float()
        idf = one_hot(ids.clamp(max=2), 3).reshape(E, 12).float()
        ei = torch.from_numpy(b.edge_index)
        y64, sigma = R.reference(cls, ctor, sd, x, ei, idf, ef)
        _REFS["keys"] = dict(y64=y64, sigma=sigma, y32=R.oracle32(cls, ctor, sd, x, ei, idf, ef), ids=ids)
    c = _REFS["keys"]
    assert torch.equal(ids, c["ids"])
    _check(c, y.cpu(), RPK, "rp keys grid %s" % grid)


def test_zz_report_largest_ratios():
    """prints, per kernel, the largest share of the factor 4 that the cases of this run used (the table of the module's docstring)"""
    for kernel in sorted(_SEEN):
        mx, rms, cases = _SEEN[kernel]
        print("RATIOS %-48s max q / max q32 %.2f   rms q / rms q32 %.2f   (%d cases)%s" % (kernel, mx, rms, cases, "   <- above 2" if max(mx, rms) > 2.0 else ""))
