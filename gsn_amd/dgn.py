"""Directional GSN (directional_gsn/): a DGN whose directional aggregators follow vector fields built from substructure counts.

The aggregation of every ``DGNLayerSimple`` (dgn_layer.py:30-56: all aggregators x scalers over the in-edges of each node) runs on one
HIP kernel family (csrc/dgn.hip, ``gsn_dgn_aggregate_fwd_hip`` / ``gsn_dgn_aggregate_bwd_hip``); the ``posttrans`` product, the BatchNorm
and the relu run on the dense stages with their native adjoints (``run_stages_autograd``); the encoders and readouts are the package's.

The classes keep the reference's constructor signatures, defaults and state-dict keys, so a reference checkpoint loads:

* :class:`DGNGraph`        -- what the reference's DGL graph carries: ``edge_index`` (row 0 source, row 1 target), ``ndata`` / ``edata``
                              (``'eig'``: the node / edge vector fields, ``'pos_enc'``), the graph of each node and ``snorm_n``.
* :class:`DGNLayerSimple`, :class:`DGNLayer` (``type_net='simple'`` only), :class:`MLPReadout`, :class:`DGNNet`.
* :func:`dgn_aggregate`    -- the differentiable aggregation on its own; :func:`avg_degree_log` -- ``avg_d['log']`` (main_HIV.py:359-363).
* :func:`laplacian_eigenvectors`, :func:`positional_encoding` -- the Laplacian eigenvector fields of data/HIV.py:21-51 (``--directions
                              eig``, ``pos_enc_dim``) for a whole batch: one launch per size class of csrc/eig.hip instead of one ARPACK
                              call per graph.

CUDA tensors only: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi
from . import _bound
from ._autograd import run_stages_autograd
from ._dense import _Stage
from ._index import _csr_for, global_add_pool_sparse, global_mean_pool_sparse
from ._runtime import _f32c, _need_cuda, _timed
from .encoding import AtomEncoder, BondEncoder

EPS = 1e-8  # aggregators.py:5

MEAN, SUM, MAX, MIN, VAR, STD, DIR_AV, DIR_SOFTMAX, DIR_DX, DIR_DX_NOABS, DIR_DX_BALANCED = range(11)   # GSN_DGN_* (gsn_abi.h)
IDENTITY, AMPLIFICATION, ATTENUATION = range(3)


def _dir_kind(name):
    """(kind, column, alpha) of a directional aggregator key of aggregators.py:74-99."""
    m = re.fullmatch(r"dir(\d+)-(av|dx|dx-no-abs|dx-balanced|0\.1|neg-0\.1)", name)
    kind = {"av": DIR_AV, "dx": DIR_DX, "dx-no-abs": DIR_DX_NOABS, "dx-balanced": DIR_DX_BALANCED,
            "0.1": DIR_SOFTMAX, "neg-0.1": DIR_SOFTMAX}[m.group(2)]
    return kind, int(m.group(1)), (-0.1 if m.group(2) == "neg-0.1" else 0.1 if m.group(2) == "0.1" else 0.0)


# The keys of the reference's AGGREGATORS (aggregators.py:74-99) and SCALERS (scalers.py:21); any other name raises KeyError, as there.
_AGG_NAMES = (["mean", "sum", "max", "min", "std", "var"] + ["dir%d-av" % c for c in range(7)] + ["dir%d-0.1" % c for c in (1, 2, 3)]
              + ["dir%d-neg-0.1" % c for c in (1, 2, 3)] + ["dir%d-dx" % c for c in range(4)] + ["dir%d-dx-no-abs" % c for c in (1, 2, 3)]
              + ["dir%d-dx-balanced" % c for c in (1, 2, 3)])
AGGREGATORS = {n: ({"mean": (MEAN, 0, 0.0), "sum": (SUM, 0, 0.0), "max": (MAX, 0, 0.0), "min": (MIN, 0, 0.0), "std": (STD, 0, 0.0),
                    "var": (VAR, 0, 0.0)}.get(n) or _dir_kind(n)) for n in _AGG_NAMES}
SCALERS = {"identity": IDENTITY, "amplification": AMPLIFICATION, "attenuation": ATTENUATION}


def _is_dir(kind):
    return kind >= DIR_AV


def parse_aggregators(names):
    """'mean max dir1-dx' (or a list of names) -> [(kind, column, alpha)]; KeyError on a name the reference does not know."""
    if isinstance(names, str):
        names = names.split()
    return [AGGREGATORS[n] for n in names]


def parse_scalers(names):
    if isinstance(names, str):
        names = names.split()
    return [SCALERS[n] for n in names]


class DGNGraph:
    """The parts of the reference's batched DGL graph a DGN reads.

    edge_index int64 [2, E] (row 0 source, row 1 target: a message flows u -> v); ``ndata['eig']`` [N, Cn] is the node field (its
    differences along each edge form the first Cn columns of the vector field), ``edata['eig']`` [E, Ce] the edge field in
    ``edge_index`` column order (the last Ce columns); ``ndata['pos_enc']`` the optional positional encoding.  ``batch`` int64 [N] is the
    graph of each node (the readout's partition) and ``snorm_n`` [N, 1] = sqrt(1 / |V(graph)|) (data/HIV.py:178-179)."""

    def __init__(self, edge_index, num_nodes, ndata=None, edata=None, batch=None, num_graphs=None, snorm_n=None, node_ptr=None,
                 edge_ptr=None):
        self.edge_index = edge_index
        self.node_ptr, self.edge_ptr = node_ptr, edge_ptr      # the graphs' vertex / edge ranges (positional_encoding reads them)
        self.num_nodes = int(num_nodes)
        self.ndata = dict(ndata or {})
        self.edata = dict(edata or {})
        dev = edge_index.device
        if batch is None:
            batch = torch.zeros(self.num_nodes, dtype=torch.int64, device=dev)
            num_graphs = 1 if num_graphs is None else num_graphs
        self.batch = batch
        self.num_graphs = int(num_graphs) if num_graphs is not None else (int(batch.max()) + 1 if batch.numel() else 0)
        if snorm_n is None:
            sizes = torch.bincount(batch, minlength=self.num_graphs).to(torch.float32).clamp(min=1.0)
            snorm_n = (1.0 / sizes)[batch].sqrt().unsqueeze(1)
        self.snorm_n = snorm_n

    def number_of_nodes(self):
        return self.num_nodes

    def number_of_edges(self):
        return int(self.edge_index.shape[1])

    @classmethod
    def from_batch(cls, batch, node_field=None, edge_field=None, device="cuda", directions=None, norm="none", pos_enc_dim=0, edge_feat=None):
        """From a collated batch (``gsn_amd.synth.Batch``: node-offset ``edge_index``, ``node_ptr``, ``edge_ptr``).

        ``directions=None``: the counts a ``counts2ids_batch`` call made for the batch (or any other field) become ``ndata['eig']`` /
        ``edata['eig']`` as float32.  ``directions`` a list: the fields are assembled in the list's order as HIVDGL.__init__ does
        (data/HIV.py:70-88) -- ``'eig'``: ``positional_encoding(g, 4, norm)``, and ``ndata['pos_enc'] = ndata['eig'][:, 1:pos_enc_dim+1]``
        when ``pos_enc_dim > 0``; ``'subgraphs'``: ``node_field`` joins ``ndata['eig']`` and ``edge_field`` joins ``edata['eig']`` (the
        reference's id_scope 'global' / 'local'; both may be given); ``'edge_feat'``: ``edge_feat`` joins ``edata['eig']``."""
        if directions is not None:
            if isinstance(directions, str):
                directions = [directions]
            for direction in directions:
                if direction not in ("eig", "subgraphs", "edge_feat"):
                    raise NotImplementedError("direction {} is not currently supported.".format(direction))     # HIV.py:82
            if "eig" in directions:
                _eig_checked_args(4, norm, 16)
                if pos_enc_dim < 0:
                    raise ValueError("pos_enc_dim = %r is negative" % (pos_enc_dim,))
            if "subgraphs" in directions and node_field is None and edge_field is None:
                raise ValueError("directions has 'subgraphs' but neither node_field nor edge_field is given")
            if "edge_feat" in directions and edge_feat is None:
                raise ValueError("directions has 'edge_feat' but edge_feat is None")
        dv = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device)
        ei = dv(batch.edge_index).to(torch.int64)
        node_ptr = _host_i64(batch.node_ptr)
        sizes = np.diff(node_ptr)
        gid = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
        snorm = np.repeat(np.sqrt(1.0 / np.maximum(sizes, 1).astype(np.float32)), sizes).astype(np.float32)
        edge_ptr = getattr(batch, "edge_ptr", None)
        g = cls(ei, int(node_ptr[-1]), batch=dv(gid), num_graphs=len(sizes), snorm_n=dv(snorm).unsqueeze(1), node_ptr=node_ptr,
                edge_ptr=None if edge_ptr is None else _host_i64(edge_ptr))
        join = lambda d, f: f if "eig" not in d else torch.cat((d["eig"], f), dim=1)
        if directions is None:
            if node_field is not None:
                g.ndata["eig"] = _as_rows(dv(node_field))
            if edge_field is not None:
                g.edata["eig"] = _as_rows(dv(edge_field))
            return g
        for direction in directions:
            if direction == "eig":
                positional_encoding(g, 4, norm)
                if pos_enc_dim > 0:
                    g.ndata["pos_enc"] = g.ndata["eig"][:, 1:pos_enc_dim + 1]
            elif direction == "subgraphs":
                if node_field is not None:
                    g.ndata["eig"] = join(g.ndata, _as_rows(dv(node_field)))
                if edge_field is not None:
                    g.edata["eig"] = join(g.edata, _as_rows(dv(edge_field)))
            else:
                g.edata["eig"] = join(g.edata, _as_rows(dv(edge_feat)))
        return g


def avg_degree_log(graphs):
    """avg_d['log'] of main_HIV.py:359-363: the mean of log(D + 1) over the nodes of the training graphs, D the in-degree (float32).
    ``graphs``: a DGNGraph, a collated batch or a list of either."""
    if not isinstance(graphs, (list, tuple)):
        graphs = [graphs]
    logs = []
    for g in graphs:
        ei = g.edge_index if isinstance(g.edge_index, torch.Tensor) else torch.from_numpy(np.asarray(g.edge_index))
        n = g.num_nodes
        D = torch.bincount(ei[1].cpu().to(torch.int64), minlength=n).to(torch.float32)
        logs.append(torch.log(D + 1))
    return torch.mean(torch.cat(logs)) if logs else torch.tensor(float("nan"))


# ------------------------------------------------------------------------------------------------------------------
# Laplacian eigenvector fields (data/HIV.py:21-51)
# ------------------------------------------------------------------------------------------------------------------
EIG_NORMS = {"none": 0, "sym": 1, "walk": 2}                     # GSN_EIG_NORM_* (gsn_abi.h)
EIG_KMAX = 8                                                      # GSN_EIG_KMAX
EIG_CLASSES = (32, 64, 128, 256)                                  # most vertices per graph of a launch (csrc/eig.hip)
EIG_MAX_SWEEPS = 64
ST_OK, ST_KEYERROR, ST_TOO_LARGE, ST_BAD_INDEX, ST_ASYMMETRIC, ST_NO_CONVERGENCE = range(6)    # GSN_ST_*


def _host_i64(a):
    """A graph-pointer array on the host (a device tensor is copied back: pass host arrays to stay asynchronous)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int64)


def _eig_checked_args(k, norm, max_sweeps):
    if norm not in EIG_NORMS:
        raise ValueError("norm = %r: the Laplacians of data/HIV.py:28-36 are 'none', 'sym' and 'walk'" % (norm,))
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= EIG_KMAX:
        raise ValueError("k = %r: 1 .. %d eigenvectors" % (k, EIG_KMAX))
    if not isinstance(max_sweeps, (int, np.integer)) or isinstance(max_sweeps, bool) or not 1 <= max_sweeps <= EIG_MAX_SWEEPS:
        raise ValueError("max_sweeps = %r: 1 .. %d" % (max_sweeps, EIG_MAX_SWEEPS))
    return int(k), EIG_NORMS[norm], int(max_sweeps)


def _raise_eig_status(status, sizes):
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if bad.size == 0:
        return
    g, code = int(bad[0]), int(st[bad[0]])
    if code == ST_ASYMMETRIC:
        raise ValueError("laplacian_eigenvectors: graph %d has an arc without its reverse (only symmetric arc sets are solved)" % g)
    if code == ST_TOO_LARGE:
        raise ValueError("laplacian_eigenvectors: graph %d has %d vertices (at most %d)" % (g, int(sizes[g]), EIG_CLASSES[-1]))
    if code == ST_BAD_INDEX:
        raise IndexError("laplacian_eigenvectors: graph %d has an edge end outside its own vertices" % g)
    raise RuntimeError("laplacian_eigenvectors: graph %d did not converge within max_sweeps (status %d)" % (g, code))


def laplacian_eigenvectors(batch, k=4, norm="none", max_sweeps=16, check=True, return_values=False, device="cuda", return_sweeps=False):
    """The ``k`` eigenvectors of smallest eigenvalue of every graph's Laplacian (data/HIV.py:21-51: 'none' D - A, 'sym'
    I - D^-1/2 A D^-1/2, 'walk' I - D^-1 A with D the in-degree clipped at 1), increasing eigenvalue: float32 [N, k] on the device.

    ``batch``: a collated batch (``node_ptr``, ``edge_ptr``, node-offset ``edge_index``; host arrays keep the call asynchronous) or a
    :class:`DGNGraph` made by ``from_batch`` (``device`` is then the graph's).  Each vector has unit 2-norm and its component of largest
    magnitude is positive (lowest vertex on ties); inside an eigenspace the choice of basis is the solver's (deterministic: two calls
    give the same bits), so compare subspaces, never elements, with another solver's output.  A graph with fewer than ``k`` vertices has
    zero vectors (NaN eigenvalues) in the missing columns.  Arc sets must be symmetric and graphs have at most 256 vertices.

    Returns ``vec`` [, ``val`` float32 [G, k] if ``return_values``] [, ``status`` int32 [G] if not ``check``] [, ``sweeps`` int32 [G] if
    ``return_sweeps``].  ``check=True`` reads the status words back once and raises ValueError (asymmetric, too large), IndexError (an
    edge end outside its graph) or RuntimeError (no convergence within ``max_sweeps`` Jacobi sweeps), naming the first such graph;
    ``check=False`` never synchronises: the graphs with a status have zero rows (no convergence: the last iterate)."""
    k, norm_code, max_sweeps = _eig_checked_args(k, norm, max_sweeps)
    if isinstance(batch, DGNGraph):
        device = batch.edge_index.device
    if batch.node_ptr is None or getattr(batch, "edge_ptr", None) is None:
        raise ValueError("laplacian_eigenvectors: the graph carries no node_ptr / edge_ptr (build it with DGNGraph.from_batch)")
    node_ptr, edge_ptr = _host_i64(batch.node_ptr), _host_i64(batch.edge_ptr)
    G = len(node_ptr) - 1
    if G < 0 or len(edge_ptr) != G + 1 or (G >= 0 and node_ptr[0] != 0) or np.any(np.diff(node_ptr) < 0) or np.any(np.diff(edge_ptr) < 0):
        raise ValueError("laplacian_eigenvectors: node_ptr / edge_ptr must be non-decreasing [G + 1] arrays starting at 0")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("laplacian_eigenvectors: device %s -- the solver is a HIP kernel and there is no CPU fallback" % (device,))
    _abi.require_gpu()
    N = int(node_ptr[-1])
    sizes = np.diff(node_ptr)
    ei = batch.edge_index if isinstance(batch.edge_index, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batch.edge_index))
    if ei.dim() != 2 or ei.shape[0] != 2 or ei.shape[1] != int(edge_ptr[-1]):
        raise ValueError("laplacian_eigenvectors: edge_index must be [2, %d] (edge_ptr[-1]), got %s" % (int(edge_ptr[-1]), list(ei.shape)))
    vec = torch.empty(N, k, dtype=torch.float32, device=device)
    val = torch.full((max(G, 0), k), float("nan"), dtype=torch.float32, device=device)
    status = torch.zeros(max(G, 0), dtype=torch.int32, device=device)
    sweeps = torch.zeros(max(G, 0), dtype=torch.int32, device=device)
    if G > 0 and N > 0:
        ei = ei.to(device=device, dtype=torch.int64).contiguous()
        E = ei.shape[1]
        npt, ept = torch.from_numpy(node_ptr).to(device), torch.from_numpy(edge_ptr).to(device)
        # one launch per size class; a graph beyond the largest class rides in the first launch, whose kernel refuses it (zero rows)
        cls_of = np.searchsorted(np.asarray(EIG_CLASSES), sizes, side="left")
        used = sorted(set(int(c) for c in cls_of if c < len(EIG_CLASSES))) or [0]
        cls_of = np.where(cls_of >= len(EIG_CLASSES), used[0], cls_of)
        with _abi.device_guard(device):
            for c in used:
                ids_h = np.flatnonzero(cls_of == c).astype(np.int32)
                ids = None if len(ids_h) == G else torch.from_numpy(ids_h).to(device)
                n_scr = int(_abi.lib().gsn_laplacian_eig_scratch_floats(EIG_CLASSES[c], len(ids_h)))
                scratch = torch.empty(n_scr, dtype=torch.float32, device=device) if n_scr else None
                with _timed("laplacian_eig_%d" % EIG_CLASSES[c], 0.0):
                    rc = _abi.lib().gsn_laplacian_eig_hip(G, _abi.ptr(npt), _abi.ptr(ept), _abi.ptr(ei) if E else None, E, _abi.ptr(ids),
                                                          len(ids_h), EIG_CLASSES[c], norm_code, k, max_sweeps, _abi.ptr(vec), _abi.ptr(val),
                                                          _abi.ptr(status), _abi.ptr(sweeps), _abi.ptr(scratch), n_scr,
                                                          _abi.current_stream())
                _abi.check(rc, "gsn_laplacian_eig_hip")
        if check:
            _raise_eig_status(status, sizes)
    out = [vec]
    if return_values:
        out.append(val)
    if not check:
        out.append(status)
    if return_sweeps:
        out.append(sweeps)
    return out[0] if len(out) == 1 else tuple(out)


def positional_encoding(g, pos_enc_dim, norm):
    """data/HIV.py:21-51 on a :class:`DGNGraph`: the ``pos_enc_dim`` Laplacian eigenvectors of smallest eigenvalue of every graph become
    (or are concatenated behind) ``g.ndata['eig']``; returns ``g``."""
    scalar_field = laplacian_eigenvectors(g, k=pos_enc_dim, norm=norm)
    g.ndata["eig"] = scalar_field if "eig" not in g.ndata else torch.cat((g.ndata["eig"], scalar_field), dim=1)
    return g


# ------------------------------------------------------------------------------------------------------------------
# the aggregation
# ------------------------------------------------------------------------------------------------------------------
class _Spec:
    """Descriptor and scaler arrays of one layer configuration, marshalled once."""

    def __init__(self, aggs, scalers, avg_log):
        self.aggs = list(aggs)
        self.n = len(self.aggs)
        self.c_aggs = (_abi.gsn_dgn_agg * self.n)(*[_abi.gsn_dgn_agg(k, c, a, i) for i, (k, c, a) in enumerate(self.aggs)])
        self.scalers = list(scalers)
        self.c_scalers = (ctypes.c_int32 * len(self.scalers))(*self.scalers)
        self.avg_log = float(avg_log)
        self.max_col = max([c for k, c, _ in self.aggs if _is_dir(k)], default=-1)


def _as_rows(f):
    """A field as a float32 [rows, columns] tensor (a 1-D field is one column)."""
    return None if f is None else _f32c(f.unsqueeze(1) if f.dim() == 1 else f)


def _fields(g_or_fields):
    nf, ef = g_or_fields
    return _as_rows(nf), _as_rows(ef)


def _field_args(nf, ef):
    return (_abi.ptr(nf) if nf is not None and nf.numel() else None, nf.stride(0) if nf is not None else 0,
            nf.shape[1] if nf is not None else 0,
            _abi.ptr(ef) if ef is not None and ef.numel() else None, ef.stride(0) if ef is not None else 0,
            ef.shape[1] if ef is not None else 0)


def _check(spec, h, edge_index, nf, ef):
    # row counts first: the kernels index the fields by node id and edge id and would read past short tensors (the reference fails
    # here too: DGL refuses ndata / edata whose first dimension is not the node / edge count)
    if h.dim() != 2 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise RuntimeError("dgn_aggregate: h must be [N, d] and edge_index [2, E] (got %s and %s)" % (list(h.shape), list(edge_index.shape)))
    N, E = h.shape[0], edge_index.shape[1]
    if nf is not None and nf.shape[0] != N:
        raise RuntimeError("node field: %d rows, expected one per node (%d)" % (nf.shape[0], N))
    if ef is not None and ef.shape[0] != E:
        raise RuntimeError("edge field: %d rows, expected one per edge (%d)" % (ef.shape[0], E))
    width = (nf.shape[1] if nf is not None else 0) + (ef.shape[1] if ef is not None else 0)
    if spec.max_col >= width:
        # vector_field[:, :, eig_idx] in the reference (aggregators.py:38-70)
        raise IndexError("index %d is out of bounds for dimension 2 with size %d (DGN vector field: %d node + %d edge columns)"
                         % (spec.max_col, width, nf.shape[1] if nf is not None else 0, ef.shape[1] if ef is not None else 0))
    _need_cuda(h, "h")
    _need_cuda(edge_index, "edge_index")
    for f, what in ((nf, "node field"), (ef, "edge field")):
        if f is not None:
            _need_cuda(f, what)


class _DGNAggregateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, edge_index, n_nodes, nf, ef, spec):
        hs = _f32c(h)
        N, d = hs.shape
        E = edge_index.shape[1]
        c = _csr_for(edge_index, 1, N)
        out = torch.empty(N, len(spec.scalers) * spec.n * d, dtype=torch.float32, device=hs.device)
        with _abi.device_guard(hs.device), _timed("dgn_aggregate_fwd", 4.0 * (N * d + E * d + out.numel())):
            rc = _abi.lib().gsn_dgn_aggregate_fwd_hip(N, E, d, _abi.ptr(c.seg_ptr), _abi.ptr(c.perm) if E else None,
                                                      _abi.ptr(c.src) if E else None, _abi.ptr(hs) if N else None, *_field_args(nf, ef),
                                                      spec.c_aggs, spec.n, spec.c_scalers, len(spec.scalers), spec.avg_log,
                                                      _abi.ptr(out) if N else None, _abi.current_stream())
        _abi.check(rc, "gsn_dgn_aggregate_fwd_hip")
        ctx.save_for_backward(hs)
        ctx.edge_index, ctx.nf, ctx.ef, ctx.spec = edge_index, nf, ef, spec
        return out

    @staticmethod
    def backward(ctx, gout):
        (hs,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        N, d = hs.shape
        ei, spec = ctx.edge_index, ctx.spec
        E = ei.shape[1]
        ct, cs = _csr_for(ei, 1, N), _csr_for(ei, 0, N)
        g = _f32c(gout)
        gmsg = torch.empty(E, d, dtype=torch.float32, device=hs.device)
        gh = torch.empty(N, d, dtype=torch.float32, device=hs.device)
        with _abi.device_guard(hs.device), _timed("dgn_aggregate_bwd", 4.0 * (N * d * 3 + E * d * 4 + g.numel())):
            rc = _abi.lib().gsn_dgn_aggregate_bwd_hip(N, E, d, _abi.ptr(ct.seg_ptr), _abi.ptr(ct.perm) if E else None,
                                                      _abi.ptr(ct.src) if E else None, _abi.ptr(cs.seg_ptr), _abi.ptr(cs.perm) if E else None,
                                                      _abi.ptr(hs) if N else None, *_field_args(ctx.nf, ctx.ef), spec.c_aggs, spec.n,
                                                      spec.c_scalers, len(spec.scalers), spec.avg_log, _abi.ptr(g) if N else None,
                                                      _abi.ptr(gmsg) if E else None, _abi.ptr(gh) if N else None, _abi.current_stream())
        _abi.check(rc, "gsn_dgn_aggregate_bwd_hip")
        return gh, None, None, None, None, None


def dgn_aggregate(h, edge_index, aggregators, scalers="identity", avg_d=None, node_field=None, edge_field=None, spec=None):
    """The reduce of DGNLayerSimple (dgn_layer.py:38-56) for every node: ``cat_s(cat_a(aggregate_a) * scale_s)`` [N, S * A * d] over
    the in-edges (u -> v) of edge_index, with vector field cat(node_field[u] - node_field[v], edge_field[e]).  As in the reference the
    scalers apply only when more than one is given; nodes without in-edges get zero rows (DGL's reduce of an empty mailbox)."""
    if spec is None:
        spec = _make_spec(aggregators, scalers, avg_d)
    nf, ef = _fields((node_field, edge_field))
    _check(spec, h, edge_index, nf, ef)
    return _DGNAggregateFn.apply(h, edge_index, h.shape[0], nf, ef, spec)


def _avg_log(avg_d):
    if avg_d is None or "log" not in avg_d:
        return 1.0
    v = avg_d["log"]
    return float(v.item() if isinstance(v, torch.Tensor) else v)


def _make_spec(aggregators, scalers, avg_d):
    aggs = parse_aggregators(aggregators)
    sc = parse_scalers(scalers)
    if len(sc) <= 1:         # dgn_layer.py:50: scaled only when more than one scaler is given
        return _Spec(aggs, [IDENTITY], 1.0)
    return _Spec(aggs, sc, _avg_log(avg_d))


# ------------------------------------------------------------------------------------------------------------------
# the reference's modules (nets/layers.py, nets/dgn_layer.py, nets/mlp_readout_layer.py, nets/HIV_graph_classification/dgn_net.py)
# ------------------------------------------------------------------------------------------------------------------
class FCLayer(nn.Module):
    """nets/layers.py:20-117 as the DGN uses it (no dropout, no BatchNorm): Linear with xavier_uniform_(W, gain=1/in_size), zero bias."""

    def __init__(self, in_size, out_size, activation="relu", dropout=0., b_norm=False, bias=True, init_fn=None, device="cpu"):
        super().__init__()
        if dropout or b_norm:
            raise NotImplementedError("FCLayer: dropout / b_norm are not used by the DGN and not supported here")
        self.in_size, self.out_size, self.bias = in_size, out_size, bias
        self.linear = nn.Linear(in_size, out_size, bias=bias)
        act = activation.lower() if isinstance(activation, str) else activation
        if act not in ("relu", "none"):
            raise NotImplementedError("FCLayer activation %r" % (activation,))
        self.activation = act
        self.init_fn = nn.init.xavier_uniform_
        self.reset_parameters()

    def reset_parameters(self, init_fn=None):
        init_fn = init_fn or self.init_fn
        if init_fn is not None:
            init_fn(self.linear.weight, 1 / self.in_size)
        if self.bias:
            self.linear.bias.data.zero_()


class MLP(nn.Module):
    """nets/layers.py:120-154: a chain of FCLayers (mid activation, last activation)."""

    def __init__(self, in_size, hidden_size, out_size, layers, mid_activation="relu", last_activation="none", dropout=0.,
                 mid_b_norm=False, last_b_norm=False, device="cpu"):
        super().__init__()
        self.in_size, self.hidden_size, self.out_size = in_size, hidden_size, out_size
        self.fully_connected = nn.ModuleList()
        if layers <= 1:
            self.fully_connected.append(FCLayer(in_size, out_size, activation=last_activation, b_norm=last_b_norm, dropout=dropout))
        else:
            self.fully_connected.append(FCLayer(in_size, hidden_size, activation=mid_activation, b_norm=mid_b_norm, dropout=dropout))
            for _ in range(layers - 2):
                self.fully_connected.append(FCLayer(hidden_size, hidden_size, activation=mid_activation, b_norm=mid_b_norm, dropout=dropout))
            self.fully_connected.append(FCLayer(hidden_size, out_size, activation=last_activation, b_norm=last_b_norm, dropout=dropout))

    def stages(self, x, post=None):
        """The chain as dense stages; ``post = (BatchNorm1d or None, activation)`` replaces the last activation."""
        out = []
        n = len(self.fully_connected)
        for i, fc in enumerate(self.fully_connected):
            bn, act = None, ("identity" if fc.activation == "none" else "relu")
            if i == n - 1 and post is not None:
                bn, act = post
            out.append(_Stage(fc.linear.weight, fc.linear.bias, bn, act, [(x, None)] if i == 0 else ()))
        return out

    def forward(self, x, post=None):
        _need_cuda(x, "mlp input")
        _bound.refuse("dgn: the MLP stages of a DGN layer")      # (DGN models are not trained on padded batches: DESIGN.md 8f)
        return run_stages_autograd(self.stages(x, post), x.shape[0], self.training)


class DGNLayerSimple(nn.Module):
    """dgn_layer.py:10-82: aggregate (HIP) -> posttrans -> [* snorm_n] -> [BatchNorm] -> relu -> [+ h_in] -> dropout.
    ``aggregators`` / ``scalers``: lists of names (or space-separated strings) -- the keys of the reference's AGGREGATORS / SCALERS."""

    def __init__(self, in_dim, out_dim, dropout, graph_norm, batch_norm, aggregators, scalers, residual, avg_d, posttrans_layers=1,
                 dropout_impl=None):
        super().__init__()
        from .dropout import resolve_impl
        self.dropout = dropout
        self.dropout_impl = resolve_impl(dropout_impl)      # "torch": F.dropout; "native": gsn_amd.dropout (None: flags.DROPOUT_NATIVE)
        self.graph_norm = graph_norm
        self.batch_norm = batch_norm
        self.residual = residual
        self.aggregators = aggregators.split() if isinstance(aggregators, str) else list(aggregators)
        self.scalers = scalers.split() if isinstance(scalers, str) else list(scalers)
        self.batchnorm_h = nn.BatchNorm1d(out_dim)
        self.posttrans = MLP(in_size=(len(self.aggregators) * len(self.scalers)) * in_dim, hidden_size=out_dim, out_size=out_dim,
                             layers=posttrans_layers, mid_activation="relu", last_activation="none")
        self.avg_d = avg_d
        self._spec = _make_spec(self.aggregators, self.scalers, avg_d)
        if in_dim != out_dim:
            self.residual = False

    def forward(self, g, h, e, snorm_n):
        h_in = h
        agg = dgn_aggregate(h, g.edge_index, None, node_field=g.ndata.get("eig"), edge_field=g.edata.get("eig"), spec=self._spec)
        if self.graph_norm:
            h = self.posttrans(agg) * snorm_n
            if self.batch_norm:
                h = self.batchnorm_h(h)
            h = F.relu(h)
        else:
            h = self.posttrans(agg, post=(self.batchnorm_h if self.batch_norm else None, "relu"))
        if self.residual:
            h = h_in + h
        if self.dropout_impl == "native":
            from .dropout import dropout as native_dropout
            return native_dropout(h, self.dropout, self.training)
        return F.dropout(h, self.dropout, training=self.training)


class DGNLayer(nn.Module):
    """dgn_layer.py:85-109.  Only ``type_net='simple'`` names a class the reference defines; ``.model`` is the layer."""

    def __init__(self, in_dim, out_dim, dropout, graph_norm, batch_norm, aggregators, scalers, avg_d, type_net, residual, towers=5,
                 divide_input=True, edge_features=None, edge_dim=None, pretrans_layers=1, posttrans_layers=1, dropout_impl=None):
        super().__init__()
        aggregators, scalers = aggregators.split(), scalers.split()
        parse_aggregators(aggregators)           # (KeyError on a name the reference does not know, as its dict lookups raise)
        parse_scalers(scalers)
        if type_net == "simple":
            self.model = DGNLayerSimple(in_dim=in_dim, out_dim=out_dim, dropout=dropout, graph_norm=graph_norm, batch_norm=batch_norm,
                                        residual=residual, aggregators=aggregators, scalers=scalers, avg_d=avg_d,
                                        posttrans_layers=posttrans_layers, dropout_impl=dropout_impl)
        else:
            raise NotImplementedError("DGNLayer type_net=%r: 'complex' and 'towers' name classes the reference never defines "
                                      "(dgn_layer.py:97-109)" % (type_net,))


class MLPReadout(nn.Module):
    """nets/mlp_readout_layer.py: L Linear + relu layers (halving widths), then Linear to output_dim."""

    def __init__(self, input_dim, output_dim, L=2, decreasing_dim=True):
        super().__init__()
        if decreasing_dim:
            fc = [nn.Linear(input_dim // 2 ** l, input_dim // 2 ** (l + 1), bias=True) for l in range(L)]
            fc.append(nn.Linear(input_dim // 2 ** L, output_dim, bias=True))
        else:
            fc = [nn.Linear(input_dim, input_dim, bias=True) for _ in range(L)]
            fc.append(nn.Linear(input_dim, output_dim, bias=True))
        self.FC_layers = nn.ModuleList(fc)
        self.L = L

    def forward(self, x):
        _need_cuda(x, "readout input")
        stages = [_Stage(lin.weight, lin.bias, None, "relu" if i < self.L else "identity", [(x, None)] if i == 0 else ())
                  for i, lin in enumerate(self.FC_layers)]
        _bound.refuse("dgn: the readout MLP")
        return run_stages_autograd(stages, x.shape[0], self.training)


class DGNNet(nn.Module):
    """nets/HIV_graph_classification/dgn_net.py: AtomEncoder -> in_feat_dropout -> [+ pos_enc Linear] -> L DGN layers -> readout
    (sum / max / mean) -> MLPReadout(out_dim, 1).  ``forward(g, h, e, snorm_n, snorm_e)``: g a DGNGraph, h the int64 [N, 9] atom codes."""

    def __init__(self, net_params):
        super().__init__()
        hidden_dim = net_params["hidden_dim"]
        out_dim = net_params["out_dim"]
        in_feat_dropout = net_params["in_feat_dropout"]
        dropout = net_params["dropout"]
        n_layers = net_params["L"]
        self.type_net = net_params["type_net"]
        self.pos_enc_dim = net_params["pos_enc_dim"]
        if self.pos_enc_dim > 0:
            self.embedding_pos_enc = nn.Linear(self.pos_enc_dim, hidden_dim)
        self.readout = net_params["readout"]
        self.graph_norm = net_params["graph_norm"]
        self.batch_norm = net_params["batch_norm"]
        self.aggregators = net_params["aggregators"]
        self.scalers = net_params["scalers"]
        self.avg_d = net_params["avg_d"]
        self.residual = net_params["residual"]
        self.edge_feat = net_params["edge_feat"]
        edge_dim = net_params["edge_dim"]
        pretrans_layers = net_params["pretrans_layers"]
        posttrans_layers = net_params["posttrans_layers"]
        self.device = net_params.get("device")
        from .dropout import Dropout as NativeDropout, resolve_impl
        self.dropout_impl = resolve_impl(net_params.get("dropout_impl"))      # "torch": nn.Dropout / F.dropout; "native": gsn_amd.dropout
        self.in_feat_dropout = NativeDropout(in_feat_dropout) if self.dropout_impl == "native" else nn.Dropout(in_feat_dropout)
        self.embedding_h = AtomEncoder(emb_dim=hidden_dim)
        if self.edge_feat:
            self.embedding_e = BondEncoder(emb_dim=edge_dim)
        mk = lambda o: DGNLayer(in_dim=hidden_dim, out_dim=o, dropout=dropout, graph_norm=self.graph_norm, batch_norm=self.batch_norm,
                                residual=self.residual, aggregators=self.aggregators, scalers=self.scalers, avg_d=self.avg_d,
                                type_net=self.type_net, edge_features=self.edge_feat, edge_dim=edge_dim, pretrans_layers=pretrans_layers,
                                posttrans_layers=posttrans_layers, dropout_impl=self.dropout_impl).model
        self.layers = nn.ModuleList([mk(hidden_dim) for _ in range(n_layers - 1)])
        self.layers.append(mk(out_dim))
        self.MLP_layer = MLPReadout(out_dim, 1)

    def forward(self, g, h, e, snorm_n, snorm_e):
        h = self.embedding_h(h)
        h = self.in_feat_dropout(h)
        if self.pos_enc_dim > 0:
            from .layers import run_linear_module
            h = h + run_linear_module(self.embedding_pos_enc, g.ndata["pos_enc"].to(h.device).float())
        if self.edge_feat:
            e = self.embedding_e(e)
        for conv in self.layers:
            h = conv(g, h, e, snorm_n)
        if self.readout == "sum":
            hg = global_add_pool_sparse(h, g.batch, g.num_graphs)
        elif self.readout == "max":
            idx = g.batch.unsqueeze(1).expand(-1, h.shape[1])
            hg = torch.zeros(g.num_graphs, h.shape[1], dtype=h.dtype, device=h.device).scatter_reduce(0, idx, h, "amax", include_self=False)
        else:
            hg = global_mean_pool_sparse(h, g.batch, g.num_graphs)    # default readout is mean nodes
        return self.MLP_layer(hg)

    def loss(self, scores, labels):
        return nn.BCEWithLogitsLoss()(scores, labels.to(scores.dtype).to(scores.device).unsqueeze(-1))
