"""Directional GSN (gsn_amd.dgn): the host-side contract, without a GPU -- names, factory paths, state-dict keys, refusals."""
import ctypes

import pytest
import torch

from helpers import load

HIV = dict(L=4, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0,
           dropout=0.3, graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av", scalers="identity", towers=5,
           divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1, posttrans_layers=1, pos_enc_dim=0,
           avg_d={"log": torch.tensor(1.2)}, device="cpu")


def _names(key):
    return [str(s) for s in load("dgn")[key]]


def test_every_reference_name_parses():
    from gsn_amd import dgn
    ref = _names("names/aggregators")
    assert sorted(ref) == sorted(dgn.AGGREGATORS)
    parsed = dgn.parse_aggregators(ref)
    assert len(parsed) == len(ref)
    for name, (kind, col, alpha) in zip(ref, parsed):
        if name.startswith("dir"):
            assert col == int(name[3]) and kind >= dgn.DIR_AV
            assert alpha == (-0.1 if "neg" in name else 0.1 if name.endswith("0.1") else 0.0)
    assert sorted(_names("names/scalers")) == sorted(dgn.SCALERS)
    assert dgn.parse_scalers(" ".join(_names("names/scalers"))) == [dgn.IDENTITY, dgn.AMPLIFICATION, dgn.ATTENUATION]


def test_unknown_names_raise_keyerror():
    from gsn_amd import dgn
    with pytest.raises(KeyError):
        dgn.parse_aggregators("mean dir7-av")
    with pytest.raises(KeyError):
        dgn.DGNLayer(8, 8, 0.0, False, True, "mean dir1-dx-foo", "identity", None, "simple", True)
    with pytest.raises(KeyError):
        dgn.DGNLayer(8, 8, 0.0, False, True, "mean", "identity squash", None, "simple", True)


@pytest.mark.parametrize("type_net", ["complex", "towers"])
def test_undefined_factory_paths_raise(type_net):
    from gsn_amd import dgn
    with pytest.raises(NotImplementedError):
        dgn.DGNLayer(8, 8, 0.0, False, True, "mean max", "identity", None, type_net, True)


def test_state_dict_keys_match_reference():
    from gsn_amd import dgn
    for pl in (1, 2):
        layer = dgn.DGNLayer(16, 16, 0.0, False, True, "mean max min dir1-dx dir1-av", "identity", None, "simple", True,
                             posttrans_layers=pl).model
        assert list(layer.state_dict()) == _names("names/layer_keys_pl%d" % pl)
    net = dgn.DGNNet(dict(HIV))
    assert list(net.state_dict()) == _names("names/net_keys")


def test_posttrans_init_and_widths():
    from gsn_amd import dgn
    torch.manual_seed(0)
    layer = dgn.DGNLayerSimple(10, 12, 0.0, False, True, ["mean", "dir1-av"], ["identity", "amplification", "attenuation"], True,
                               {"log": 1.0}, posttrans_layers=1)
    w = layer.posttrans.fully_connected[0].linear
    assert w.weight.shape == (12, 2 * 3 * 10) and float(w.bias.abs().max()) == 0.0
    bound = (1 / 60) * (6.0 / (60 + 12)) ** 0.5                 # xavier_uniform_(W, gain=1/in_size) (nets/layers.py:94-99)
    assert float(w.weight.abs().max()) <= bound
    assert layer.residual is False                              # in_dim != out_dim


def test_single_scaler_is_not_applied():
    from gsn_amd import dgn
    spec = dgn._make_spec("mean", "amplification", {"log": 2.0})
    assert spec.scalers == [dgn.IDENTITY]                       # dgn_layer.py:50: len(self.scalers) > 1
    spec = dgn._make_spec("mean", "identity amplification", {"log": 2.0})
    assert spec.scalers == [dgn.IDENTITY, dgn.AMPLIFICATION] and spec.avg_log == 2.0


def test_cpu_tensors_refused():
    from gsn_amd import dgn
    h = torch.randn(4, 3)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(RuntimeError, match="CPU fallback"):
        dgn.dgn_aggregate(h, ei, "mean max")
    g = dgn.DGNGraph(ei, 4, edata={"eig": torch.randn(3, 2)})
    layer = dgn.DGNLayerSimple(3, 3, 0.0, False, True, ["mean", "dir1-av"], ["identity"], True, None)
    with pytest.raises(RuntimeError, match="CPU fallback"):
        layer(g, h, None, g.snorm_n)


def test_field_column_out_of_range_refused():
    from gsn_amd import dgn
    h = torch.randn(4, 3)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(IndexError):                              # 2 edge columns: dir2 does not exist (the reference's IndexError)
        dgn.dgn_aggregate(h, ei, "mean dir2-av", edge_field=torch.randn(3, 2))
    with pytest.raises(IndexError):
        dgn.dgn_aggregate(h, ei, "dir0-dx", node_field=None, edge_field=None)
    with pytest.raises(IndexError):
        dgn.dgn_aggregate(h, ei, "dir3-dx", node_field=torch.randn(4, 1), edge_field=torch.randn(3, 2))


def test_field_row_counts_refused():
    """A field indexed by node id / edge id must have one row per node / edge: the kernels would read past a short tensor (e.g. the
    [N, C] vertex counts passed as the edge field)."""
    from gsn_amd import dgn
    h = torch.randn(4, 3)
    ei = torch.tensor([[0, 1, 2, 3, 0], [1, 2, 3, 0, 2]])
    with pytest.raises(RuntimeError, match="edge field: 4 rows, expected one per edge \\(5\\)"):
        dgn.dgn_aggregate(h, ei, "mean dir0-av", edge_field=torch.randn(4, 2))       # vertex counts passed as the edge field
    with pytest.raises(RuntimeError, match="node field: 5 rows, expected one per node \\(4\\)"):
        dgn.dgn_aggregate(h, ei, "mean dir0-av", node_field=torch.randn(5, 2))       # edge counts passed as the node field
    with pytest.raises(RuntimeError, match="node field: 3 rows"):
        dgn.dgn_aggregate(h, ei, "dir0-dx", node_field=torch.randn(3, 1), edge_field=torch.randn(5, 1))
    g = dgn.DGNGraph(ei, 4, edata={"eig": torch.randn(4, 2)})
    layer = dgn.DGNLayerSimple(3, 3, 0.0, False, True, ["mean", "dir1-av"], ["identity"], True, None)
    with pytest.raises(RuntimeError, match="edge field"):
        layer(g, h, None, g.snorm_n)


def test_native_entry_refuses_bad_column_before_launch():
    """The C entry checks the columns against the field widths on the host: no device, no launch needed to refuse."""
    from gsn_amd import _abi
    L = _abi.lib()
    aggs = (_abi.gsn_dgn_agg * 2)(_abi.gsn_dgn_agg(0, 0, 0.0, 0), _abi.gsn_dgn_agg(8, 3, 0.0, 1))
    sc = (ctypes.c_int32 * 1)(0)
    field = (ctypes.c_float * 8)()              # (never read: zero nodes)
    rc = L.gsn_dgn_aggregate_fwd_hip(0, 0, 4, None, None, None, None, None, 0, 0, ctypes.addressof(field), 2, 2, aggs, 2, sc, 1, 1.0,
                                     None, None)
    assert rc == -1 and b"field column 3" in L.gsn_last_error()
    aggs[1].col = 2
    rc = L.gsn_dgn_aggregate_fwd_hip(0, 0, 4, None, None, None, None, None, 0, 0, ctypes.addressof(field), 2, 2, aggs, 2, sc, 1, 1.0,
                                     None, None)
    assert rc == -1 and b"field column 2" in L.gsn_last_error()
    aggs[1].col = 1
    rc = L.gsn_dgn_aggregate_fwd_hip(0, 0, 4, None, None, None, None, None, 0, 0, ctypes.addressof(field), 2, 2, aggs, 2, sc, 1, 1.0,
                                     None, None)
    assert rc == 0                                               # column 1 of a 2-column field, zero nodes: nothing to do
    rc = L.gsn_dgn_aggregate_fwd_hip(0, 5, 4, None, None, None, None, None, 0, 0, None, 2, 2, aggs, 2, sc, 1, 1.0, None, None)
    assert rc == -1 and b"bad field" in L.gsn_last_error()      # 5 edges, edge width 2, but no edge field pointer
