"""Datasets, models and comparisons shared by tests/test_padded_loader_gpu.py and tests/test_graphed_epoch_gpu.py (made once per process):
the 32 ZINC-shaped prepared graphs and the GNNSubstructures of tests/test_loader_gpu.py::test_model_and_evaluation_over_a_loader, and a
molhiv-shaped toy (multi-feature atoms and bonds, 20 % NaN labels, a last single-vertex graph) with a small GNN_OGB with virtual node."""
import functools

import networkx as nx
import numpy as np
import torch

from gsn_amd.data import Data

DEV = "cuda"


def within_bar(a, b):
    """the project's element-wise bar: |a - b| <= 1e-5 |b| + 1e-5 max|b row|"""
    a, b = a.detach().double().cpu().reshape(b.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    bar = 1e-5 * b.abs() + 1e-5 * b.abs().max(dim=1, keepdim=True).values
    return bool(((a - b).abs() <= bar).all())


def same_bytes(a, b):
    """dtype, shape and every byte (NaN payloads included: torch.equal calls NaN unequal to itself)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.numel() == 0 or torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@functools.lru_cache(maxsize=None)
def zinc_graphs():
    from gsn_amd import synth
    from gsn_amd.counting import counts2ids_batch
    b = synth.zinc_shape_batch(32, seed=77)
    pats = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
    ids = counts2ids_batch(b, pats, "edge", False, device=DEV).cpu().clamp(max=2)
    rng = np.random.default_rng(7)
    graphs = []
    for g in range(b.num_graphs):
        n0, n1, e0, e1 = int(b.node_ptr[g]), int(b.node_ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        d = Data()
        d.edge_index = torch.from_numpy(b.edge_index[:, e0:e1] - n0)
        d.x = torch.from_numpy(b.atom_type[n0:n1]).unsqueeze(1)
        d.graph_size = n1 - n0
        d.degrees = torch.zeros(n1 - n0)
        d.edge_features = torch.from_numpy(b.bond_type[e0:e1]).unsqueeze(1)
        d.y = torch.from_numpy(rng.standard_normal(1).astype(np.float32))
        d.identifiers = ids[e0:e1].clone()
        graphs.append(d)
    return graphs


def zinc_model(seed=0):
    from gsn_amd import models
    from test_model_gpu import _kwargs
    kw = _kwargs("GSN_edge_sparse", 3, 32, "general", "local", True, False, "mean", "relu", False, "one_hot_encoder", "one_hot_encoder",
                 "one_hot_encoder", 16)
    torch.manual_seed(seed)
    return models.GNNSubstructures(1, 1, None, [3, 3, 3, 3], 1, [28], [4], **kw).to(DEV).eval()


def zinc_code_model(seed=0, L=2, d=128):
    """the shape of scripts/train_step_zinc.py's model: one projection behind the last layer, so that layer 0 runs on integer codes (its
    code-gather stages carry an out-of-range flag that an eager forward reads back)"""
    from gsn_amd import models
    kw = dict(seed=0, model_name="GSN_edge_sparse", readout="sum", dropout_features=[0.0] * (L + 1), bn=[True] * L,
              final_projection=[False] * L + [True], inject_ids=False, inject_edge_features=True, random_features=False,
              id_scope="local", d_msg=[d] * L, d_out=[d] * L, d_h=[[d]] * L, aggr="add", flow="source_to_target",
              msg_kind="general", train_eps=[False] * L, activation_mlp="relu", bn_mlp=True, jk_mlp=True, degree_embedding="None",
              degree_as_tag=[False] * L, retain_features=[True] * L, multi_embedding_aggr="sum", input_node_encoder="one_hot_encoder",
              d_out_node_encoder=d, edge_encoder="one_hot_encoder", d_out_edge_encoder=[d] * L, id_embedding="one_hot_encoder",
              d_out_id_embedding=d, d_out_degree_embedding=d, extend_dims=True, activation="relu")
    torch.manual_seed(seed)
    return models.GNNSubstructures(1, 1, None, [3, 3, 3, 3], 1, [28], [4], None, None, **kw).to(DEV).eval()


ATOM_DIMS, BOND_DIMS, ID_DIMS = [7, 3, 4], [4, 2], [3, 5]


@functools.lru_cache(maxsize=None)
def molhiv_graphs(n_graphs=25, single_vertex_last=True):
    """molhiv-shaped toy: n_graphs molecule-shaped graphs (the last one a single vertex without edges), integer atom / bond / identifier
    codes, one 0 / 1 label per graph of which 20 % are NaN"""
    from gsn_amd import synth
    b = synth.zinc_shape_batch(n_graphs, seed=5, mean_n=14.0, sd_n=5.0, n_min=3, n_max=30)
    rng = np.random.default_rng(11)
    graphs = []
    for g in range(n_graphs):
        n0, n1, e0, e1 = int(b.node_ptr[g]), int(b.node_ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        ei = b.edge_index[:, e0:e1] - n0
        if single_vertex_last and g == n_graphs - 1:
            n1, ei = n0 + 1, np.zeros((2, 0), dtype=np.int64)
        n, E = n1 - n0, ei.shape[1]
        d = Data()
        d.edge_index = torch.from_numpy(np.ascontiguousarray(ei.astype(np.int64)))
        d.x = torch.from_numpy(np.stack([rng.integers(0, k, n) for k in ATOM_DIMS], 1).astype(np.int64))
        d.degrees = torch.zeros(n)
        d.edge_features = torch.from_numpy(np.stack([rng.integers(0, k, E) for k in BOND_DIMS], 1).astype(np.int64).reshape(E, len(BOND_DIMS)))
        d.identifiers = torch.from_numpy(np.stack([rng.integers(0, k, E) for k in ID_DIMS], 1).astype(np.int64).reshape(E, len(ID_DIMS)))
        label = float(rng.integers(0, 2))
        d.y = torch.tensor([[float("nan") if rng.random() < 0.2 else label]], dtype=torch.float32)
        graphs.append(d)
    labels = torch.cat([g.y for g in graphs]).reshape(-1)
    assert bool(torch.isnan(labels).any()) and bool((labels == 0).any()) and bool((labels == 1).any())
    return graphs


def ogb_model(seed=0, L=2, dm=32):
    from gsn_amd import models
    kw = dict(seed=0, model_name="GSN_edge_sparse_ogb", readout="mean", dropout_features=[0.0] * (L + 1), bn=[True] * L,
              final_projection=[False] * L + [True], residual=False, inject_ids=True, vn=True, id_scope="local",
              d_msg=[dm] * L, d_out=[dm] * L, d_h=[[2 * dm]] * L, aggr="add", flow="source_to_target", msg_kind="ogb",
              train_eps=[True] * L, activation_mlp="relu", bn_mlp=True, jk_mlp=False, degree_embedding="None",
              degree_as_tag=[False] * L, retain_features=[True] * L, multi_embedding_aggr="sum", features_scope="full",
              input_node_encoder="embedding", d_out_node_encoder=dm, input_vn_encoder="embedding", d_out_vn_encoder=dm,
              edge_encoder="embedding", d_out_edge_encoder=[dm] * L, id_embedding="embedding", d_out_id_embedding=dm,
              d_out_degree_embedding=dm, d_out_vn=[dm] * (L - 1), vn_pooling="sum", extend_dims=True, activation="relu")
    torch.manual_seed(seed)
    model = models.GNN_OGB(len(ATOM_DIMS), 1, None, ID_DIMS, len(BOND_DIMS), ATOM_DIMS, BOND_DIMS, None, None, **kw).to(DEV).eval()
    # BatchNorm statistics that are not the identity, as after training
    g = torch.Generator().manual_seed(seed + 1)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return model
