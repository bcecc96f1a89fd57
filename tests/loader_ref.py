"""Referee of the device-resident loader (gsn_amd/loader.py): what torch_geometric's collate does, in pure torch on the CPU, and the fixture
datasets of tests/test_loader_cpu.py and tests/test_loader_gpu.py, from numpy alone.  All comparisons against it are exact."""
import numpy as np
import torch

from gsn_amd.data import Data

ATTR_ORDER = ("edge_index", "x", "graph_size", "degrees", "edge_features", "y", "identifiers")      # prepare_graphs' order (dataset.py:157-181)


def collate_ref(graphs, indices):
    """The batch of ``[graphs[i] for i in indices]``: per attribute ``torch.cat`` over the chosen graphs (``edge_index`` along dimension 1,
    raised by the running row count of ``x``; int / float attributes and 0-d tensors stacked to ``[B]``), plus ``batch``, ``ptr``,
    ``edge_ptr`` (int64 [B + 1]) and ``num_graphs``."""
    chosen = [graphs[int(i)] for i in indices]
    out = Data()
    names = [k for k, _ in chosen[0]]
    n = torch.tensor([int(g.x.shape[0]) for g in chosen], dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(n, 0)])
    for name in names:
        vals = [getattr(g, name) for g in chosen]
        v0 = vals[0]
        if isinstance(v0, int):
            t = torch.tensor(vals, dtype=torch.int64)
        elif isinstance(v0, float):
            t = torch.tensor(vals, dtype=torch.float32)
        elif v0.dim() == 0:
            t = torch.stack(vals)
        elif name == "edge_index":
            t = torch.cat([v + ptr[j] for j, v in enumerate(vals)], dim=1)
        else:
            t = torch.cat(vals, dim=0)
        setattr(out, name, t)
    out.batch = torch.repeat_interleave(torch.arange(len(chosen), dtype=torch.int64), n)
    out.ptr = ptr
    if "edge_index" in names:
        e = torch.tensor([int(g.edge_index.shape[1]) for g in chosen], dtype=torch.int64)
        out.edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(e, 0)])
    out.num_graphs = len(chosen)
    return out


def _random_edges(rng, n, m):
    """int64 [2, 2 m]: m random vertex pairs (repeats and self loops kept) in both directions, shuffled"""
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    both = np.concatenate([np.stack([u, v]), np.stack([v, u])], axis=1)
    return both[:, rng.permutation(both.shape[1])].astype(np.int64)


def _graph(rng, variant, n, ei, short_degrees=False):
    E = ei.shape[1]
    t = torch.from_numpy
    d = Data()
    d.edge_index = t(np.ascontiguousarray(ei))
    if variant == "A":
        d.x = t(rng.integers(0, 28, (n, 1)).astype(np.int64))
    else:
        d.x = t(rng.standard_normal((n, 5)).astype(np.float32))                  # 20-byte rows
    d.graph_size = int(n)
    n_deg = max(n - 3, 0) if short_degrees else n
    d.degrees = t(rng.integers(0, 5, n_deg).astype(np.float32))
    d.edge_features = t(rng.integers(0, 4, E).astype(np.int64))                  # 1-D
    if variant == "A":
        d.y = t(rng.standard_normal(1).astype(np.float32))
        d.identifiers = t(rng.integers(0, 9, (E, 5)).astype(np.int64))           # edge mode
    else:
        d.y = t(rng.standard_normal((1, 3)).astype(np.float32))
        d.identifiers = t(rng.integers(0, 9, (n, 3)).astype(np.int64))           # vertex mode
        d.coords = t(rng.standard_normal((n, 2)))                                # float64
        d.tags = t(rng.integers(-5, 5, (E, 3)).astype(np.int32))                 # int32, 12-byte rows
    return d


def make_dataset(seed, variant):
    """Fixture datasets.  'A' / 'B': the same 40 graphs of 1 - 70 vertices -- graph 3 has one vertex, graphs 7 and 19 no edges (19's
    ``edge_index`` an empty tensor reshaped to [2, 0]), graph 11's ``degrees`` is three rows shorter than its ``x`` -- with the attributes of
    an edge-mode (A) or a vertex-mode (B) prepared dataset; B adds a float64 and an int32 field.  'long': six tiny graphs and one of 3 000
    vertices / 10 000 edge columns.  'many': 5 000 graphs of 1 - 3 vertices."""
    rng = np.random.default_rng(seed)
    graphs = []
    if variant in ("A", "B"):
        srng = np.random.default_rng(seed)                   # the shapes: shared by A and B
        for g in range(40):
            n = 1 if g == 3 else (70 if g == 5 else int(srng.integers(2, 71)))
            m = 0 if g in (3, 7, 19) else int(srng.integers(1, 2 * n))
            ei = _random_edges(srng, n, m) if m else np.zeros((2, 0), dtype=np.int64)
            d = _graph(rng, variant, n, ei, short_degrees=(g == 11))
            if g == 19:
                d.edge_index = torch.empty(0, dtype=torch.int64).reshape(2, 0)
            graphs.append(d)
        assert graphs[11].degrees.shape[0] < graphs[11].x.shape[0]
    elif variant == "long":
        for g in range(7):
            n, m = (3000, 5000) if g == 4 else (int(rng.integers(1, 5)), int(rng.integers(0, 4)))
            ei = _random_edges(rng, n, m) if m else np.zeros((2, 0), dtype=np.int64)
            graphs.append(_graph(rng, "A", n, ei))
    elif variant == "many":
        for g in range(5000):
            n = int(rng.integers(1, 4))
            m = int(rng.integers(0, 3))
            ei = _random_edges(rng, n, m) if m else np.zeros((2, 0), dtype=np.int64)
            graphs.append(_graph(rng, "A", n, ei))
    else:
        raise ValueError(variant)
    return graphs


def assert_batch_equal(got, want, where=""):
    """Every attribute of the referee batch ``want`` is in ``got`` with the same dtype, shape and values (device tensors are copied back)."""
    for name, w in want:
        g = getattr(got, name)
        if isinstance(w, torch.Tensor):
            g = torch.from_numpy(g) if isinstance(g, np.ndarray) else g.cpu()      # (edge_ptr: a host array on a loader's batch)
            assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
            assert torch.equal(g, w), (where, name)
        else:
            assert g == w, (where, name, g, w)
