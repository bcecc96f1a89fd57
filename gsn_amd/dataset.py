"""Batched preprocessing driver: the reference's ``generate_dataset`` / ``_prepare`` (utils_data_gen.py:17-108) with ONE
counting launch per dataset shard instead of one Python call per graph and pattern.

What stays identical to the reference, graph by graph: the attributes each prepared graph carries and their order
(``edge_index`` without self loops, ``x``, ``graph_size``, ``degrees``, ``edge_features`` filtered in lock-step, ``y``,
``identifiers`` int64 [rows, sum orbits] with columns in pattern order then orbit index -- utils_ids.py:7-29), the
returned tuple, the ``.pt`` cache tuple ``(graphs, num_classes, orbit_partition_sizes)`` (utils.py:272-274) and
``downgrade_k`` slicing (utils.py:332-345).  Collation of the raw graphs is host-side numpy; the counts come from the
HIP kernels (gsn_count_hip; gsn_count_sparse_hip for graphs of more than 768 vertices, directed or not) -- there is no CPU counting path here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import counting, data as gdata, dist
from .patterns import PatternGraph


_WIDTH_CLASSES = np.array([64, 128, 256, 512, 768])      # vertices: the LDS kernel's bit rows of 1 / 2 / 4 / 8 / 12 words; above: the sparse kernel


def _mode_of(count_fn):
    name = count_fn if isinstance(count_fn, str) else getattr(count_fn, "__name__", "")
    if name in ("subgraph_isomorphism_edge_counts", "edge"):
        return "edge"
    if name in ("subgraph_isomorphism_vertex_counts", "vertex"):
        return "vertex"
    raise TypeError("count_fn must be subgraph_isomorphism_vertex_counts or subgraph_isomorphism_edge_counts")


def _label_tensor(label, as_float):
    t = label.detach().clone() if isinstance(label, torch.Tensor) else torch.tensor(label)
    t = t.unsqueeze(0)
    return t.float() if as_float else t.long()


def prepare_graphs(graphs, subgraph_dicts, subgraph_params, regression, dataset_name, count_fn, data_cls=None,
                   device=None, shard=None):
    """``[_prepare(g, ...) for g in graphs]`` (utils_data_gen.py:86-108) with all counting done in one launch.

    ``graphs``: records with ``edge_mat`` int64 [2,E], ``node_features`` [n, ...], ``label`` and optionally
    ``edge_features`` [E, ...] (what the loaders of :mod:`gsn_amd.data` return).  ``shard=(rank, world)`` prepares only this
    rank's cost-balanced contiguous chunk (graphs are independent, no collective) and returns
    ``(prepared, (lo, hi))`` instead of the list.

    Two deviations, both where the reference raises by accident: a zero-edge graph in edge mode gets the empty
    ``[0, sum orbits]`` identifier matrix the reference intends (its line :104 dies on an undefined name), and
    ``directed=True`` with the EDGE counter is refused up front (NameError in the reference,
    utils_graph_processing.py:146 vs :164); ``directed=True`` vertex counts treat every column of ``edge_mat`` as an arc."""
    mode = _mode_of(count_fn)
    directed = bool(subgraph_params.get("directed", False))
    if directed and mode == "edge":
        raise NotImplementedError("directed=True is not supported by the edge counter")
    data_cls = data_cls or gdata.Data
    pats = []
    for d in subgraph_dicts:
        sg = d["subgraph"]
        if not isinstance(sg, PatternGraph):
            raise TypeError("subgraph_dicts must come from gsn_amd's automorphism functions")
        pats.append(sg)
    dirorb = any(p.directed_orbits for p in pats) if mode == "edge" else False
    directed = counting._directed_of(pats, directed)
    # (wide=True: patterns of 10 to 16 vertices give a wide table, which count_batch sends to the sparse kernel whatever the width class)
    plan = counting.CountPlan.get([p.edge_list for p in pats], mode, subgraph_params["induced"], dirorb, directed, wide=True)

    span = (0, len(graphs))
    if shard is not None:
        rank, world = shard
        # sum_v deg(v)^(k-1) per graph, k = the largest pattern (self loops / duplicates included: a proxy)
        kmax = max(p.num_vertices() for p in pats)
        cost = np.array([float(dist.counting_cost(g.edge_mat.reshape(2, -1).numpy(), [0, g.edge_mat.reshape(2, -1).shape[1]], kmax)[0])
                         for g in graphs])
        bounds = dist.shard_by_cost(cost, world)
        span = (int(bounds[rank]), int(bounds[rank + 1]))
        graphs = graphs[span[0]:span[1]]

    # Width classes.  The counting kernel's instantiation follows the LARGEST graph of a launch (bit rows of 1 / 2 / 4 / 8 / 12 words: 64 ..
    # 768 vertices), so one 222-vertex molecule would put all 41 k graphs of ogbg-molhiv (25 vertices on average) on the four-word kernel
    # instead of the molecule kernel (two graphs per wave, compile-time invariants).  Graphs are independent: they are processed grouped by
    # class -- one launch per class that occurs, each over a contiguous range of the regrouped batch -- and handed back in the caller's order.
    # Graphs of more than 768 vertices are a class of their own: the LDS-resident kernel does not take them, the sparse kernel
    # (gsn_count_sparse_hip) counts them in a launch of its own.  A class whose launch the LDS kernel refuses for its size all the same
    # (tables beyond its LDS, 65 535 columns in a graph) is repeated on the sparse kernel (count_batch: large="sparse").  A wide plan
    # (patterns of 10 to 16 vertices) puts every class on the sparse kernel, still one launch per class.
    order = None
    if len(graphs) > 1:
        cls = np.searchsorted(_WIDTH_CLASSES, np.array([int(g.node_features.shape[0]) for g in graphs]), side="left")
        if cls.min() != cls.max():
            order = np.argsort(cls, kind="stable")
            graphs = [graphs[int(i)] for i in order]
    G = len(graphs)
    n_nodes = np.array([int(g.node_features.shape[0]) for g in graphs], dtype=np.int64)
    n_raw = np.array([int(g.edge_mat.shape[1]) for g in graphs], dtype=np.int64)
    node_ptr = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    raw_ptr = np.concatenate([[0], np.cumsum(n_raw)]).astype(np.int64)
    if G and raw_ptr[-1]:
        ei_raw = torch.cat([g.edge_mat.reshape(2, -1).to(torch.int64) for g in graphs], 1).numpy()
    else:
        ei_raw = np.zeros((2, 0), dtype=np.int64)
    gid = np.repeat(np.arange(G), n_raw)
    keep = ei_raw[0] != ei_raw[1]
    ei = np.ascontiguousarray(ei_raw[:, keep])
    n_kept = np.bincount(gid[keep], minlength=G).astype(np.int64) if G else np.zeros(0, np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(n_kept)]).astype(np.int64)

    # degrees = torch_geometric.utils.degree(edge_mat[0]) BEFORE self-loop removal; without num_nodes its length is
    # max(source id)+1, so trailing vertices that never occur as a source are cut (utils_data_gen.py:93-96)
    if ei_raw.shape[1]:
        deg_all = np.bincount(node_ptr[gid] + ei_raw[0], minlength=int(node_ptr[-1])).astype(np.float32)
        max_src = np.full(G, -1, dtype=np.int64)
        np.maximum.at(max_src, gid, ei_raw[0])
    else:
        deg_all = np.zeros(int(node_ptr[-1]), dtype=np.float32)
        max_src = np.full(G, -1, dtype=np.int64)

    n_cols = plan.n_cols

    def by_falling_cost(lo, hi):
        """Graphs of more than 64 vertices take a workgroup each, and a launch ends when its slowest workgroup does: handing the graphs out by
        falling estimated cost (sum_v deg(v)^(k-1), SURVEY.md 8(e)'s proxy) starts the long searches first -- BASELINE config 5 at 2 048 graphs per
        launch: 53.3 k -> 55.1 k graphs/s (scripts/gpu/r6_er_order.py).  Molecule-size graphs share a wave in pairs: left in their order."""
        if hi - lo < 2 or n_nodes[lo:hi].max() <= 64:
            return None
        kmax = max(p.num_vertices() for p in pats)
        w = deg_all.astype(np.float64) ** (kmax - 1)
        csum = np.concatenate([[0.0], np.cumsum(w)])
        cost = csum[node_ptr[lo + 1:hi + 1]] - csum[node_ptr[lo:hi]]
        return np.argsort(-cost, kind="stable").astype(np.int32)

    if G and (mode == "vertex" or edge_ptr[-1] > 0):
        if order is None:
            out, _ = counting.count_batch(plan, node_ptr, edge_ptr, torch.from_numpy(ei), ids_are_global=False,
                                          max_nodes=int(max(n_nodes.max(), 1)), max_edges=int(n_kept.max()), device=device,
                                          graph_ids=by_falling_cost(0, G), large="sparse")
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            ei_d = torch.from_numpy(ei).to(dev)
            out = torch.empty((int(node_ptr[-1]) if mode == "vertex" else int(edge_ptr[-1]), n_cols), dtype=torch.int64, device=dev)
            cls_sorted = np.searchsorted(_WIDTH_CLASSES, n_nodes, side="left")
            for c in np.unique(cls_sorted):
                lo, hi = int(np.searchsorted(cls_sorted, c, side="left")), int(np.searchsorted(cls_sorted, c, side="right"))
                if mode == "edge" and edge_ptr[hi] == edge_ptr[lo]:
                    continue
                counting.count_batch(plan, node_ptr[lo:hi + 1], edge_ptr[lo:hi + 1], ei_d, ids_are_global=False,
                                     max_nodes=int(max(n_nodes[lo:hi].max(), 1)), max_edges=int(n_kept[lo:hi].max()), device=dev, out=out,
                                     graph_ids=by_falling_cost(lo, hi), large="sparse")
        ids_all = out.cpu()
    else:
        ids_all = torch.zeros((0, n_cols), dtype=torch.int64)
    row_ptr = node_ptr if mode == "vertex" else edge_ptr
    ei_t = torch.from_numpy(ei)
    keep_t = torch.from_numpy(keep)

    as_float = bool(regression) or dataset_name in {"ogbg-molpcba", "ogbg-molhiv", "ZINC"}
    prepared = []
    for g, src in enumerate(graphs):
        d = data_cls()
        has_edges = n_raw[g] > 0
        untouched = (not has_edges) and mode == "edge"      # the reference skips the id extraction for these
        if untouched:
            setattr(d, "edge_index", src.edge_mat)
        else:
            setattr(d, "edge_index", ei_t[:, edge_ptr[g]:edge_ptr[g + 1]].clone())
        setattr(d, "x", src.node_features)
        setattr(d, "graph_size", int(n_nodes[g]))
        if not has_edges:
            setattr(d, "degrees", torch.zeros((int(n_nodes[g]),)))
        else:
            lo = int(node_ptr[g])
            setattr(d, "degrees", torch.from_numpy(deg_all[lo:lo + int(max_src[g]) + 1].copy()))
        if hasattr(src, "edge_features"):
            ef = src.edge_features
            if not untouched:
                ef = ef[keep_t[raw_ptr[g]:raw_ptr[g + 1]]]
            setattr(d, "edge_features", ef)
        setattr(d, "y", _label_tensor(src.label, as_float))
        if untouched:
            setattr(d, "identifiers", torch.zeros((0, n_cols)).long())
        else:
            setattr(d, "identifiers", ids_all[int(row_ptr[g]):int(row_ptr[g + 1])].clone())
        prepared.append(d)
    if order is not None:
        back = [None] * G
        for j, i in enumerate(order):
            back[int(i)] = prepared[j]
        prepared = back
    if shard is not None:
        return prepared, span
    return prepared


def generate_dataset(data_path, dataset_name, k, extract_ids_fn, count_fn, automorphism_fn, regression, id_type,
                     multiprocessing=False, num_processes=1, **subgraph_params):
    """Same signature and return tuple as utils_data_gen.py:17-81:
    ``(graphs_ptg, num_classes, num_node_type, num_edge_type, orbit_partition_sizes)``.

    ``extract_ids_fn`` / ``multiprocessing`` / ``num_processes`` are accepted and have no effect: the identifier
    extraction is batched inside (one launch for the whole dataset), which is what the worker pool was for."""
    if "edge_list" not in subgraph_params:
        raise ValueError("Edge list not provided.")
    subgraph_dicts, orbit_partition_sizes = [], []
    for edge_list in subgraph_params["edge_list"]:
        subgraph, orbit_partition, orbit_membership, aut_count = automorphism_fn(
            edge_list=edge_list, directed=subgraph_params["directed"], directed_orbits=subgraph_params["directed_orbits"])
        subgraph_dicts.append({"subgraph": subgraph, "orbit_partition": orbit_partition,
                               "orbit_membership": orbit_membership, "aut_count": aut_count})
        orbit_partition_sizes.append(len(orbit_partition))
    graphs, num_classes, num_node_type, num_edge_type = gdata.load_raw(data_path, dataset_name)
    data_cls = subgraph_params.get("data_cls")
    graphs_ptg = prepare_graphs(graphs, subgraph_dicts, subgraph_params, regression, dataset_name, count_fn, data_cls=data_cls)
    return graphs_ptg, num_classes, num_node_type, num_edge_type, orbit_partition_sizes


def downgrade_k(dataset, k, orbit_partition_sizes, k_min):
    """Keep only the identifier columns of the patterns up to size ``k`` (utils.py:332-345)."""
    width = sum(orbit_partition_sizes[0:k - k_min + 1])
    out = []
    for d in dataset:
        nd = type(d)()
        for name, value in d:
            setattr(nd, name, value)
        setattr(nd, "identifiers", d.identifiers[:, 0:width])
        out.append(nd)
    return out, orbit_partition_sizes[0:k - k_min + 1]


def save_dataset(graphs_ptg, num_classes, orbit_partition_sizes, data_file):
    """The reference's cache tuple (utils.py:256, :274)."""
    torch.save((graphs_ptg, num_classes, orbit_partition_sizes), data_file)


def load_dataset(data_file):
    """utils.py:277-287."""
    obj = torch.load(data_file, weights_only=False)
    return obj[0], obj[1], obj[2]
