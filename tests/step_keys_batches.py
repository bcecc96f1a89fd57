"""Batches and layers shared by tests/test_step_keys_gpu.py: ZINC-shaped molecules and hand-made multigraphs (duplicate columns, self loops,
isolated vertices, a hub) in the construction style of tests/test_step_gpu.py."""
import networkx as nx
import numpy as np
import torch


def cycles(ks=range(3, 7)):
    return [list(nx.cycle_graph(k).edges) for k in ks]


def ctor(d_in=28, d_ef=4, d_id=12):
    return dict(d_in=d_in, d_ef=d_ef, d_id=d_id, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128,
                d_up=128, d_h=[128], seed=0, activation_name="relu", bn=True, msg_kind="general")


def make_layer(flow, seed=0, **widths):
    from gsn_amd import layers
    torch.manual_seed(seed)
    layer = layers.GSN_edge_sparse(flow=flow, **ctor(**widths)).to(torch.device("cuda", 0)).eval()
    with torch.no_grad():                                               # running statistics that are not the identity
        for m in layer.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    return layer


def both_directions(u, v, rng):
    """Columns (u, v) and (v, u) of undirected pairs -- repeats and self loops kept -- in no particular order."""
    both = np.concatenate([np.stack([u, v]), np.stack([v, u])], 1)
    return both[:, rng.permutation(both.shape[1])].astype(np.int64)


def hand_made_graphs(seed=5):
    """(n, edge_index) per graph, graph-local ids: random multigraphs with self loops and repeated columns; two graphs without any column (60
    consecutive vertices without an in-edge: with one wave range per ~28 nodes a whole tile whose only block is empty); a hub whose 35 leaves
    are each named twice (in-degree 70: a tile of few nodes, three blocks); and a tail that makes E no multiple of 32."""
    rng = np.random.default_rng(seed)
    graphs = []
    for g in range(9):
        n = int(rng.integers(2, 30))
        m = int(rng.integers(1, 40))
        graphs.append((n, both_directions(rng.integers(0, n, m), rng.integers(0, n, m), rng)))
    empty = np.zeros((2, 0), dtype=np.int64)
    graphs += [(30, empty), (30, empty)]
    leaves = np.arange(1, 36)
    graphs.append((36, both_directions(np.concatenate([leaves, leaves]), np.zeros(70, dtype=np.int64), rng)))
    graphs.append((5, both_directions(np.array([0, 1, 2, 2]), np.array([1, 2, 2, 4]), rng)))       # (vertex 3 has no in-edge; a self loop on 2)
    graphs.append((3, both_directions(np.array([0]), np.array([1]), rng)))
    return graphs


def collate_to_device(graphs):
    from gsn_amd import synth
    b = synth.collate(graphs)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).to(dev)
    return b, t(b.node_ptr), t(b.edge_ptr), t(b.edge_index)
