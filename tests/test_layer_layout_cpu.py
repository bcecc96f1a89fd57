"""The message-row layout of the `general` layers and the one-launch eligibility rule, each stated once in gsn_amd.layers
(``_SparseLayer._row`` -> ``_MessageRow``, ``_SparseLayer._one_launch_shape``), against the order written out literally here:
``cat(x[i], x[j], ids  or  ids[i], ids[j], ef)`` -- the rows graph_filters/GSN_sparse.py:166-171 and GSN_edge_sparse.py:160-165 build.
Small CPU tensors: the helper only arranges its arguments."""
import types

import pytest
import torch

from gsn_amd import layers
from gsn_amd.step import CountLayerStep

CLASSES = ["GSN_sparse", "GSN_edge_sparse", "MPNN_sparse", "MPNN_edge_sparse", "GSN_edge_sparse_ogb", "MPNN_edge_sparse_ogb"]
D_X, D_ID, D_EF, N = 5, 3, 2, 9


def _layer(cls, scope="local", flow="source_to_target", d_h=(8,), kind=None):
    ogb = cls.endswith("_ogb")
    kw = dict(d_in=D_X, d_degree=1, degree_as_tag=False, retain_features=True, d_msg=8, d_up=8, d_h=list(d_h), seed=0, activation_name="relu",
              bn=True, flow=flow, msg_kind=kind or ("ogb" if ogb else "general"))
    if cls.startswith("GSN"):
        kw.update(d_id=D_X if ogb else D_ID, id_scope=scope)
    if "edge" in cls:
        kw.update(d_ef=D_X if ogb else D_EF)
    if kind == "gin":
        kw.update(id_embedding="one_hot_encoder", edge_embedding="one_hot_encoder", extend_dims=True)
    torch.manual_seed(0)
    return getattr(layers, cls)(**kw)


def _inputs(layer, scope, E):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, D_X, generator=g)
    ids = torch.randn(N if scope == "global" else E, D_ID, generator=g) if layer.has_ids else None
    ef = torch.randn(E, D_EF, generator=g) if layer.has_ef else None
    ei = torch.randint(0, N, (2, E), generator=g)
    return x, ids, ef, ei


def _gathered(blocks):
    return torch.cat([t if idx is None else t[idx.long()] for t, idx in blocks], -1)


@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
@pytest.mark.parametrize("scope", ["local", "global"])
@pytest.mark.parametrize("cls", CLASSES)
def test_blocks_are_the_reference_row(cls, scope, flow):
    layer = _layer(cls, scope, flow)
    E = 14
    x, ids, ef, ei = _inputs(layer, scope, E)
    # the reference's row, written out: i is the aggregating end (edge_index[1] for source_to_target, GSN_sparse.py:134-139)
    i, j = (ei[1], ei[0]) if flow == "source_to_target" else (ei[0], ei[1])
    parts = [x[i], x[j]]
    if layer.has_ids:
        parts += [ids] if scope == "local" else [ids[i], ids[j]]
    if layer.has_ef:
        parts.append(ef)
    want = torch.cat(parts, -1)
    sel = layer._sel()
    assert torch.equal(ei[sel], i) and torch.equal(ei[1 - sel], j)
    row = layer._row(x, ids, ef)
    # (1) through the edge_index rows
    assert torch.equal(_gathered(row.blocks(ei[sel], ei[1 - sel], None)), want)
    # (2) through a target-sorted CSR's int32 indices (sorted target, sorted source, permutation): the same rows in sorted order
    perm = torch.sort(i, stable=True).indices
    tgt, src = i[perm].int(), j[perm].int()
    assert torch.equal(_gathered(row.blocks(tgt, src, perm.int())), want[perm])
    # (3) as the gather modes of the training path: block b through edge_index[mode], None = one row per edge
    tensors, modes = zip(*row.blocks(sel, 1 - sel, None))
    assert torch.equal(_gathered([(t, None if m is None else ei[m]) for t, m in zip(tensors, modes)]), want)
    # which inputs are per vertex and which per edge
    per_node_ids = layer.has_ids and scope == "global"
    assert [t is x for t in row.node[:1]] == [True] and len(row.node) == (2 if per_node_ids else 1)
    assert all(t.shape[0] == N for t in row.node) and all(t.shape[0] == E for t in row.edge)
    assert len(row.edge) == int(layer.has_ids and not per_node_ids) + int(layer.has_ef)
    assert layer._ids_per_node() == per_node_ids
    # the columns of msg_fn's first weight per block
    cols = row.columns()
    assert [b - a for a, b in cols] == [t.shape[1] for t, _ in row.blocks(None, None, None)]
    assert cols[0][0] == 0 and all(cols[k][1] == cols[k + 1][0] for k in range(len(cols) - 1)) and cols[-1][1] == want.shape[1]
    if layer.msg_kind == "general":
        w1 = layer.msg_fn.fc[0].weight.detach()
        assert w1.shape[1] == want.shape[1]
        assert torch.equal(torch.cat([w1[:, a:b] for a, b in cols], 1), w1)
        per_block = sum(_gathered([blk]) @ w1[:, a:b].t() for blk, (a, b) in zip(row.blocks(i, j, None), cols))
        assert torch.allclose(per_block, want @ w1.t(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("cls,scope,d_h,kind,want", [
    ("GSN_edge_sparse", "local", (8,), None, True), ("GSN_sparse", "local", (8,), None, True),
    ("MPNN_sparse", None, (8,), None, True), ("MPNN_edge_sparse", None, (8,), None, True),
    ("GSN_edge_sparse", "global", (8,), None, False), ("GSN_sparse", "global", (8,), None, False),
    ("GSN_edge_sparse", "local", (8, 8), None, False), ("GSN_edge_sparse", "local", (), None, False),
    ("GSN_edge_sparse", "local", (8,), "gin", False), ("GSN_sparse", "global", (8,), "gin", False),
    ("GSN_edge_sparse_ogb", "local", (8,), None, False), ("MPNN_edge_sparse_ogb", None, (8,), None, False)])
def test_one_launch_shape(cls, scope, d_h, kind, want):
    assert _layer(cls, scope, d_h=d_h, kind=kind)._one_launch_shape() is want


@pytest.mark.parametrize("cls,scope,d_h,kind", [
    ("GSN_edge_sparse", "global", (8,), None), ("GSN_sparse", "global", (8,), None), ("MPNN_edge_sparse", None, (8,), None),
    ("GSN_edge_sparse", "local", (8, 8), None), ("GSN_edge_sparse", "local", (8,), "gin"), ("GSN_edge_sparse_ogb", "local", (8,), None)])
def test_count_layer_step_refuses_what_it_refused(cls, scope, d_h, kind):
    plan = types.SimpleNamespace(mode="edge", n_cols=2)
    with pytest.raises(ValueError, match="CountLayerStep: a `general` GSN_edge_sparse layer with id_scope='local' and a two-stage msg_fn"):
        CountLayerStep(plan, _layer(cls, scope, d_h=d_h, kind=kind), [3, 3])


def test_count_layer_step_takes_the_local_two_stage_layer():
    plan = types.SimpleNamespace(mode="edge", n_cols=2)
    step = CountLayerStep(plan, _layer("GSN_edge_sparse", "local"), [3, 3])
    assert step.layer.has_ids and step.layer._one_launch_shape()
