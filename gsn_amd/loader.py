"""Device-resident dataset and DataLoader: the reference's ``for data in loader`` (train_test_funcs.py:48-174, a
``torch_geometric.data.DataLoader`` over the list ``prepare_graphs`` returns) with the dataset kept on the GPU and every collated batch made
by ONE HIP launch (``gsn_loader_collate_hip``, csrc/loader.hip).

* :class:`DeviceDataset` -- the prepared graphs as one device tensor per attribute (a *field*: the concatenation over all graphs) with an
  int64 row pointer per field; fields with equal row pointers share a *pointer class*.  ``edge_index`` is the one special field: stored
  ``[2, E_total]`` with graph-local vertex ids, raised in a batch by the vertices of the graphs in front of it (PyG's ``__inc__``).
* :class:`DataLoader`    -- sequential or shuffled batches.  Per EPOCH: the order and, per pointer class, the rows in front of every position
  inside its own batch (the *plan*, a cumulative sum that restarts at batch boundaries) go to the device in one asynchronous copy from
  pinned memory.  Per BATCH: output allocations through torch, one kernel launch; no host-to-device copy, no synchronisation.
* :class:`Batch`         -- what ``next()`` returns: every field under its own name plus ``batch``, ``ptr``, ``num_graphs``, the host pointers
  ``node_ptr`` / ``edge_ptr`` and ``graph_partition`` (exact sizes: ``models._register_partition`` needs no device read).

* :class:`PaddedDataLoader` / :class:`PaddedBatch` -- the same batches collated into ONE set of static, fixed-capacity tensors
  (``gsn_loader_collate_padded_hip``), filled up with whole *pad graphs*: shapes and pointers never change, so an EVALUATION step over them
  can be captured into a HIP graph once and replayed per batch (``evaluation.GraphedEpoch``).

Batches of :class:`DataLoader` have variable shapes: they are not for capture into a HIP graph.  Padded batches are for ``model.eval()``
only (padding rows would enter train-mode BatchNorm statistics; the models refuse them in training mode).
There is no CPU path: the host code here validates, sizes and plans; the rows are moved by the kernel only.
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np
import torch

from . import _abi
from .data import Data

GSN_LOADER_MAX_FIELDS = 16
_KIND_COPY, _KIND_EDGE_INDEX = 0, 1
_F_NODES, _F_PAD_EDGES, _F_PAD_GRAPH = 1, 2, 4
_DTYPES = {torch.int64: 8, torch.int32: 4, torch.float32: 4, torch.float64: 8}
_NODE_FIELD, _EDGE_FIELD = "x", "edge_index"


class _Field:
    """One attribute of the dataset: its storage (host until uploaded), dtype, trailing shape and pointer class."""
    __slots__ = ("name", "kind", "dtype", "trailing", "scalar", "python", "cls", "storage", "row_bytes", "elem_bytes", "row_ptr_dev")

    def __init__(self, name, kind, dtype, trailing, scalar, python):
        self.name, self.kind, self.dtype, self.trailing, self.scalar, self.python = name, kind, dtype, trailing, scalar, python
        self.cls = -1
        self.storage = None
        self.row_ptr_dev = None
        self.elem_bytes = _DTYPES[dtype]
        n = 1
        for s in trailing:
            n *= int(s)
        self.row_bytes = self.elem_bytes * n if kind == _KIND_COPY else 8


def _describe(name, value, g):
    """(kind, dtype, trailing shape, rows, scalar, python type or None) of attribute ``name`` of graph ``g``; raises on what cannot be a field"""
    if isinstance(value, bool):
        raise TypeError("DeviceDataset: attribute %r of graph %d is a bool (tensors of int64 / int32 / float32 / float64, int or float)" % (name, g))
    if isinstance(value, int):
        return _KIND_COPY, torch.int64, (), 1, True, int
    if isinstance(value, float):
        return _KIND_COPY, torch.float32, (), 1, True, float
    if not isinstance(value, torch.Tensor):
        raise TypeError("DeviceDataset: attribute %r of graph %d is a %s (tensors, int or float)" % (name, g, type(value).__name__))
    if value.dtype not in _DTYPES:
        raise TypeError("DeviceDataset: attribute %r of graph %d has dtype %s (int64, int32, float32 or float64)" % (name, g, value.dtype))
    if name == _EDGE_FIELD:
        if value.dtype is not torch.int64 or value.dim() != 2 or value.shape[0] != 2:
            raise (TypeError if value.dtype is not torch.int64 else ValueError)(
                "DeviceDataset: edge_index of graph %d is %s %s (int64 [2, E])" % (g, value.dtype, list(value.shape)))
        return _KIND_EDGE_INDEX, torch.int64, (), int(value.shape[1]), False, None
    if value.dim() == 0:
        return _KIND_COPY, value.dtype, (), 1, True, None
    return _KIND_COPY, value.dtype, tuple(value.shape[1:]), int(value.shape[0]), False, None


def _assemble(graphs, validate):
    """Host half of DeviceDataset: (fields with host storage, class sizes int64 [C][G], per-graph python scalars).  Runs without a GPU."""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("DeviceDataset: no graphs")
    names = [k for k, _ in graphs[0]]
    if len(names) > GSN_LOADER_MAX_FIELDS:
        raise ValueError("DeviceDataset: %d attributes (at most GSN_LOADER_MAX_FIELDS = %d fields)" % (len(names), GSN_LOADER_MAX_FIELDS))
    G = len(graphs)
    fields, parts, sizes = [], [], []
    for name in names:
        parts.append([None] * G)
        sizes.append(np.zeros(G, dtype=np.int64))
    for g, d in enumerate(graphs):
        items = list(d)
        got = [k for k, _ in items]
        if got != names:
            odd = sorted(set(got) ^ set(names)) or got
            raise ValueError("DeviceDataset: graph %d has attributes %s, graph 0 has %s (attribute %r)" % (g, got, names, odd[0]))
        for j, (name, value) in enumerate(items):
            kind, dtype, trailing, rows, scalar, python = _describe(name, value, g)
            if g == 0:
                fields.append(_Field(name, kind, dtype, trailing, scalar, python))
            f = fields[j]
            if dtype is not f.dtype or python is not f.python:
                raise TypeError("DeviceDataset: attribute %r of graph %d is %s, of graph 0 %s" % (name, g, python.__name__ if python else dtype,
                                                                                            f.python.__name__ if f.python else f.dtype))
            if trailing != f.trailing or scalar != f.scalar:
                raise ValueError("DeviceDataset: attribute %r of graph %d has rows of shape %s, of graph 0 %s" % (name, g, list(trailing), list(f.trailing)))
            parts[j][g] = value
            sizes[j][g] = rows
    by_name = {f.name: j for j, f in enumerate(fields)}
    if _NODE_FIELD not in by_name or fields[by_name[_NODE_FIELD]].scalar:
        raise ValueError("DeviceDataset: the graphs need a tensor attribute 'x' (its rows are the vertices)")
    n_nodes = sizes[by_name[_NODE_FIELD]]
    for j, f in enumerate(fields):
        if f.python is not None:
            f.storage = torch.tensor(parts[j], dtype=f.dtype)
        elif f.scalar:
            f.storage = torch.stack(parts[j])
        elif f.kind == _KIND_EDGE_INDEX:
            f.storage = torch.cat(parts[j], dim=1).contiguous()
            if validate and f.storage.shape[1]:
                owner = np.repeat(np.arange(G), sizes[j])
                ei = f.storage.numpy()
                bad = (ei < 0) | (ei >= n_nodes[owner][None, :])
                if bad.any():
                    g = int(owner[np.nonzero(bad.any(axis=0))[0][0]])
                    raise ValueError("DeviceDataset: edge_index of graph %d names a vertex outside [0, %d)" % (g, int(n_nodes[g])))
        else:
            f.storage = torch.cat(parts[j], dim=0).contiguous()
    classes = []
    for j, f in enumerate(fields):
        for c, s in enumerate(classes):
            if np.array_equal(s, sizes[j]):
                f.cls = c
                break
        else:
            f.cls = len(classes)
            classes.append(sizes[j])
    scalars = {f.name: parts[j] for j, f in enumerate(fields) if f.python is not None}
    return fields, np.stack(classes), scalars


class _Storage:
    """What a dataset and its subsets share: the device fields, their row pointers (device and host) and the host sizes per class."""

    def __init__(self, fields, sizes, scalars, device):
        self.fields, self.sizes, self.scalars, self.device = fields, sizes, scalars, device
        self.by_name = {f.name: f for f in fields}
        self.node_cls = self.by_name[_NODE_FIELD].cls
        self.edge_field = self.by_name.get(_EDGE_FIELD)
        self.edge_cls = self.edge_field.cls if self.edge_field is not None else -1
        C, G = sizes.shape
        self.row_ptr = np.zeros((C, G + 1), dtype=np.int64)
        np.cumsum(sizes, axis=1, out=self.row_ptr[:, 1:])
        row_ptr_dev = torch.from_numpy(self.row_ptr).to(device)
        for f in fields:
            f.storage = f.storage.to(device)
            f.row_ptr_dev = row_ptr_dev[f.cls]


class DeviceDataset:
    """A list of ``Data``-like graphs (what ``dataset.prepare_graphs`` returns) held on the device.

    Attributes are read by iterating each graph as ``data.Data.__iter__`` does, in the first graph's order; every graph must carry the same
    names.  A tensor attribute is a field of ``t.shape[0]`` rows per graph (a 0-d tensor: one row), with one dtype (int64, int32, float32,
    float64) and one trailing shape over the dataset; row counts are whatever the graphs hold (``degrees`` may be shorter than ``x``).
    ``edge_index`` is int64 ``[2, E_g]`` with graph-local ids; with ``validate`` every value is checked once, on the host, to lie in
    ``[0, rows of x)`` -- the kernels that consume a batch's ``graph_partition`` trust that.  ``int`` / ``float`` attributes become
    graph-level fields (int64 / float32).  ``len(ds)``, ``ds[i]`` (a ``Data`` of device views, ``edge_index`` local) and ``ds.subset(idx)``
    (the same device storage restricted to ``idx``: the splits of a dataset share one copy)."""

    def __init__(self, graphs, device=None, validate=True):
        fields, sizes, scalars = _assemble(graphs, validate)
        _abi.require_gpu()
        _abi.lib()
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise RuntimeError("gsn_amd.loader: device %s; the dataset lives on the GPU (no CPU fallback)" % (device,))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._st = _Storage(fields, sizes, scalars, device)
        self._index = np.arange(sizes.shape[1], dtype=np.int64)

    @property
    def device(self):
        return self._st.device

    @property
    def field_names(self):
        return [f.name for f in self._st.fields]

    def field_storage(self, name):
        """The device tensor that holds attribute ``name`` of every graph of the underlying storage (shared by subsets)."""
        return self._st.by_name[name].storage

    def host_sizes(self, name):
        """numpy int64 [len(self)]: the rows of attribute ``name`` per graph"""
        return self._st.sizes[self._st.by_name[name].cls][self._index]

    def __len__(self):
        return len(self._index)

    def subset(self, indices):
        idx = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < -len(self) or idx.max() >= len(self)):
            raise IndexError("DeviceDataset.subset: index outside [0, %d)" % len(self))
        sub = object.__new__(DeviceDataset)
        sub._st = self._st
        sub._index = self._index[idx]
        return sub

    def __getitem__(self, i):
        if isinstance(i, (slice, list, tuple, np.ndarray, torch.Tensor)):
            return self.subset(np.arange(len(self))[i] if isinstance(i, slice) else i)
        g = int(self._index[int(i)])
        st = self._st
        d = Data()
        for f in st.fields:
            lo, hi = int(st.row_ptr[f.cls, g]), int(st.row_ptr[f.cls, g + 1])
            if f.python is not None:
                v = st.scalars[f.name][g]
            elif f.scalar:
                v = f.storage[lo]
            elif f.kind == _KIND_EDGE_INDEX:
                v = f.storage[:, lo:hi]
            else:
                v = f.storage[lo:hi]
            setattr(d, f.name, v)
        return d


class Batch(Data):
    """A collated batch on the device.  ``to(device)`` is the identity for the batch's own device."""

    def to(self, device):
        dev = torch.device(device) if not isinstance(device, torch.device) else device
        own = self._device
        if dev.type == own.type and (dev.index is None or dev.index == own.index):
            return self
        return super().to(device)


def epoch_plan(sizes, order, batch_size, drop_last=False):
    """Host plan of an epoch.  ``sizes`` int64 [C, G_storage] (rows per pointer class and graph), ``order`` int64 [P] (the graph at every
    position).  Returns ``(plan, totals, n_batches)``: ``plan`` int64 [C, P], the class-c rows in front of position i inside its own batch (a
    cumulative sum that restarts at every multiple of ``batch_size``); ``totals`` int64 [C, n_batches], the rows of every batch.  With
    ``drop_last`` the positions behind the last full batch belong to no batch (their plan entries are those of the partial batch)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    order = np.asarray(order, dtype=np.int64)
    P = int(order.shape[0])
    bs = int(batch_size)
    if bs < 1:
        raise ValueError("batch_size = %r" % (batch_size,))
    C = sizes.shape[0]
    s = sizes[:, order] if P else np.zeros((C, 0), dtype=np.int64)
    incl = np.cumsum(s, axis=1)
    excl = incl - s
    starts = np.arange(0, P, bs)
    plan = excl - np.repeat(excl[:, starts], np.minimum(bs, P - starts), axis=1) if P else excl
    n_batches = P // bs if drop_last else (P + bs - 1) // bs
    totals = np.add.reduceat(s, starts, axis=1)[:, :n_batches] if P else np.zeros((C, 0), dtype=np.int64)
    return np.ascontiguousarray(plan), np.ascontiguousarray(totals), n_batches


class _Epoch:
    """Iterator over one epoch.  Owns the epoch's device table (row 0: the order, rows 1 ..: the plan) and, until its copy has completed,
    the pinned buffer it was staged in (torch's pinned allocator does not reuse a block while a copy from it is pending)."""

    def __init__(self, loader, order, shared=None):
        ds = loader.dataset
        st = ds._st
        self.loader, self.st = loader, st
        bs = loader.batch_size
        ids = ds._index[order]                                 # storage ids in epoch order
        if shared is None:
            plan, totals, n_batches = epoch_plan(st.sizes, ids, bs, loader.drop_last)
            C, P = plan.shape
            staged = torch.empty((C + 1, max(P, 1)), dtype=torch.int64, pin_memory=True)
            host = staged.numpy()
            host[0, :P] = ids
            host[1:, :P] = plan
            table = torch.empty((C + 1, max(P, 1)), dtype=torch.int64, device=st.device)
            table.copy_(staged, non_blocking=True)
            self._staged = staged
            s = st.sizes[:, ids]
            starts = np.arange(0, P, bs)[:n_batches]
            node_max = np.maximum.reduceat(s[st.node_cls], starts) if n_batches else np.zeros(0, dtype=np.int64)
            edge_max = (np.maximum.reduceat(s[st.edge_cls], starts) if n_batches else np.zeros(0, dtype=np.int64)) if st.edge_cls >= 0 else None
            if loader.drop_last and n_batches and P > n_batches * bs:      # (reduceat's last group runs to the end of the row)
                lo = (n_batches - 1) * bs
                node_max[-1] = s[st.node_cls, lo:lo + bs].max()
                if edge_max is not None:
                    edge_max[-1] = s[st.edge_cls, lo:lo + bs].max()
            shared = (table, plan, totals, n_batches, node_max, edge_max, P)
        self.shared = shared
        self.table, self.plan, self.totals, self.n_batches, self.node_max, self.edge_max, self.P = shared
        self.stride = int(self.table.shape[1])
        self.b = 0
        # the launch's field table: everything but the destinations is fixed for the epoch
        self.rec = (_abi.gsn_loader_field * len(st.fields))()
        for r, f in zip(self.rec, st.fields):
            r.src, r.row_ptr = f.storage.data_ptr(), f.row_ptr_dev.data_ptr()
            r.row_bytes, r.elem_bytes, r.ptr_class, r.kind = f.row_bytes, f.elem_bytes, f.cls, f.kind
            r.inc_class = st.node_cls
            r.src_stride = int(f.storage.shape[1]) if f.kind == _KIND_EDGE_INDEX else 0
            r.flags = _F_NODES if f.name == _NODE_FIELD else 0
        self.order_ptr = self.table.data_ptr()
        self.plan_ptr = self.table[1:].data_ptr()

    def __iter__(self):
        return self

    def __len__(self):
        return self.n_batches - self.b

    def __next__(self):
        b = self.b
        if b >= self.n_batches:
            raise StopIteration
        self.b = b + 1
        st, bs = self.st, self.loader.batch_size
        first = b * bs
        B = min(bs, self.P - first)
        dev = st.device
        out = Batch()
        out._device = dev
        totals = self.totals[:, b]
        with _abi.device_guard(dev):
            for r, f in zip(self.rec, st.fields):
                rows = int(totals[f.cls])
                if f.kind == _KIND_EDGE_INDEX:
                    t = torch.empty((2, rows), dtype=torch.int64, device=dev)
                    r.dst_stride = rows
                elif f.scalar:
                    t = torch.empty((rows,), dtype=f.dtype, device=dev)
                else:
                    t = torch.empty((rows,) + f.trailing, dtype=f.dtype, device=dev)
                r.dst, r.dst_rows = (t.data_ptr() if rows else None), rows
                setattr(out, f.name, t)
            n_b = int(totals[st.node_cls])
            batch_vec = torch.empty((n_b,), dtype=torch.int64, device=dev)
            ptrs = torch.empty((2, B + 1), dtype=torch.int64, device=dev)
            ptr, edge_ptr_dev = ptrs[0], ptrs[1]
            has_edges = st.edge_cls >= 0
            _abi.check(_abi.lib().gsn_loader_collate_hip(len(self.rec), self.rec, self.order_ptr, self.plan_ptr, self.stride, first, B,
                                                         batch_vec.data_ptr() if n_b else None, ptr.data_ptr(),
                                                         edge_ptr_dev.data_ptr() if has_edges else None, _abi.current_stream()), "gsn_loader_collate_hip")
        out.batch = batch_vec
        out.ptr = ptr
        out.num_graphs = B
        node_ptr = np.empty(B + 1, dtype=np.int64)
        node_ptr[:B] = self.plan[st.node_cls, first:first + B]
        node_ptr[B] = n_b
        out.node_ptr = node_ptr
        if has_edges:
            edge_ptr = np.empty(B + 1, dtype=np.int64)
            edge_ptr[:B] = self.plan[st.edge_cls, first:first + B]
            edge_ptr[B] = int(totals[st.edge_cls])
            out.edge_ptr = edge_ptr
            out.graph_partition = (ptr, edge_ptr_dev, int(self.node_max[b]), int(self.edge_max[b]), False)
        return out


class EpochOrder:
    """The order of an epoch, drawn on the host: ``arange(n)``, or ``torch.randperm(n, generator=generator)`` -- with ``generator=None`` from
    a private ``torch.Generator`` seeded once, here, from ``torch.initial_seed()``."""

    def __init__(self, shuffle=False, generator=None):
        self.shuffle = bool(shuffle)
        if self.shuffle and generator is None:
            generator = torch.Generator()
            generator.manual_seed(torch.initial_seed())
        self.generator = generator

    def draw(self, n):
        return torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)


class DataLoader:
    """Batches of a :class:`DeviceDataset` (a list of ``Data`` is wrapped into one), one HIP launch each.

    ``shuffle=False``: positions ``arange(G)``; ``shuffle=True``: ``torch.randperm(G, generator=generator)`` drawn on the CPU at every
    ``__iter__`` -- with ``generator=None`` from a private ``torch.Generator`` seeded once from ``torch.initial_seed()``.  The order of the
    epoch started last is ``loader.last_permutation`` (host int64).  NO promise is made of matching the order of
    ``torch.utils.data.DataLoader`` (or torch_geometric's) under the same seed: only that every epoch is a permutation of the dataset and
    that the same generator state gives the same sequence.

    Every ``__iter__`` starts an epoch with its own plan on the device; iterators of one loader may be alive together
    (``zip(loader, loader)``), and a batch stays valid and unchanged after later batches and epochs have been drawn."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, generator=None):
        if not isinstance(dataset, DeviceDataset):
            dataset = DeviceDataset(dataset)
        if not isinstance(batch_size, (int, np.integer)) or isinstance(batch_size, bool) or batch_size < 1:
            raise ValueError("DataLoader: batch_size = %r" % (batch_size,))
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self._order = EpochOrder(self.shuffle, generator)
        self.generator = self._order.generator
        self.last_permutation = None
        self._sequential = None                  # shuffle=False: the one plan of the loader, uploaded once

    def __len__(self):
        G = len(self.dataset)
        return G // self.batch_size if self.drop_last else (G + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        perm = self._order.draw(len(self.dataset))
        self.last_permutation = perm
        if self.shuffle:
            return _Epoch(self, perm.numpy())
        ep = _Epoch(self, perm.numpy(), self._sequential)
        self._sequential = ep.shared
        return ep


from ._bound import RowBound, masked_training  # noqa: E402,F401  (the training-mode opt-in for padded batches: DESIGN.md 8f)


# ---- padded, fixed-shape batches ----------------------------------------------------------------------------------------------------
class PaddedShape:
    """The static shape of a padded loader: ``n_chunk`` / ``e_chunk`` (the most vertices / edge columns of a pad graph), ``node_capacity``,
    ``edge_capacity``, ``pad_slots`` (P) and ``graph_slots`` (G_cap = batch_size + P)."""
    __slots__ = ("batch_size", "n_chunk", "e_chunk", "node_capacity", "edge_capacity", "pad_slots", "graph_slots")

    def __repr__(self):
        return "PaddedShape(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k in self.__slots__)


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def padded_shape(n_sizes, e_sizes, batch_size, shuffle=False, drop_last=False, node_capacity=None, edge_capacity=None):
    """Host arithmetic of a padded loader over graphs of ``n_sizes`` vertices and ``e_sizes`` edge columns (int arrays [G], in dataset
    order).  ``n_chunk = max(n_max, 2)``, ``e_chunk = max(e_max, 1)``: a pad graph is never larger than the dataset's largest graph.
    Default capacities hold every batch the loader can draw -- sequential: of its own batches; shuffled: of the ``batch_size`` largest
    graphs -- and ``node_capacity`` adds the vertices of the pad graphs that use up what a smaller batch leaves:
    ``N_cap = M + max(1, ceil(M / (n_chunk - 1)), ceil(E_cap / e_chunk))`` with M the most ``N_r + batch_size - b`` of a batch."""
    n = np.asarray(n_sizes, dtype=np.int64).reshape(-1)
    e = np.asarray(e_sizes, dtype=np.int64).reshape(-1)
    G, B = int(n.shape[0]), int(batch_size)
    if G < 1 or e.shape[0] != G or B < 1:
        raise ValueError("padded_shape: %d graphs, %d edge counts, batch_size %d" % (G, e.shape[0], B))
    sh = PaddedShape()
    sh.batch_size = B
    sh.n_chunk, sh.e_chunk = max(int(n.max()), 2), max(int(e.max()), 1)
    if shuffle:
        k = min(B, G)
        m = int(np.sort(np.maximum(n, 1))[G - k:].sum()) + B - k
        e_need = int(np.sort(e)[G - k:].sum())
    else:
        starts = np.arange(0, G, B)
        b = np.minimum(B, G - starts)
        n_tot, e_tot = np.add.reduceat(n, starts) + B - b, np.add.reduceat(e, starts)
        if drop_last and G >= B:                      # (the partial batch is never drawn)
            n_tot, e_tot = n_tot[b == B], e_tot[b == B]
        m, e_need = int(n_tot.max()), int(e_tot.max())
    sh.edge_capacity = e_need if edge_capacity is None else int(edge_capacity)
    if sh.edge_capacity < 0:
        raise ValueError("padded_shape: edge_capacity = %r" % (edge_capacity,))
    if node_capacity is None:
        sh.node_capacity = m + max(1, _ceil_div(m, sh.n_chunk - 1), _ceil_div(sh.edge_capacity, sh.e_chunk))
    else:
        sh.node_capacity = int(node_capacity)
    if sh.node_capacity < 1:
        raise ValueError("padded_shape: node_capacity = %r" % (node_capacity,))
    sh.pad_slots = max(1, _ceil_div(sh.node_capacity, sh.n_chunk), _ceil_div(sh.edge_capacity, sh.e_chunk))
    sh.graph_slots = B + sh.pad_slots
    return sh


def padded_fits(sh, b, n_real_nodes, n_real_edges):
    """A batch of ``b`` graphs fits iff every pad slot can have its vertex and the real edge columns do not pass the capacity."""
    return int(n_real_nodes) + sh.graph_slots - int(b) <= sh.node_capacity and int(n_real_edges) <= sh.edge_capacity


def pad_pointers(sh, b, n_real_nodes, n_real_edges):
    """``(node_ptr, edge_ptr)`` int64 [S + 1] of the S = graph_slots - b pad graphs of a batch that fits: pad graph k has
    ``1 + min(n_chunk - 1, max(0, r_n - k (n_chunk - 1)))`` vertices and ``min(e_chunk, max(0, r_e - k e_chunk))`` edge columns
    (``r_n = N_cap - N_r - S``, ``r_e = E_cap - E_r``); the last entries are the capacities."""
    S = sh.graph_slots - int(b)
    k = np.arange(S + 1, dtype=np.int64)
    r_n, r_e = sh.node_capacity - int(n_real_nodes) - S, sh.edge_capacity - int(n_real_edges)
    return int(n_real_nodes) + k + np.minimum(r_n, k * (sh.n_chunk - 1)), int(n_real_edges) + np.minimum(r_e, k * sh.e_chunk)


class PaddedBatch(Batch):
    """A padded batch: ``num_graphs = G_cap`` graph slots of which the first ``num_real_graphs`` are real (``num_real_nodes`` vertices,
    ``num_real_edges`` edge columns; ``n_valid``: the same count on the device).  The tensors BELONG TO THE LOADER and are refilled by the
    next batch: copy what must outlive it.  Real rows are always a prefix -- vertices ``[0, N_r)``, edge columns ``[0, E_r)``, graphs
    ``[0, b)`` -- and the three bounds are on the device (``n_valid`` = b, ``ptr[b]`` = N_r, ``graph_partition[1][b]`` = E_r): what
    :func:`masked_training` hands to the train-mode BatchNorm kernels."""
    padded = True


_NP_OF = {torch.int64: np.int64, torch.int32: np.int32, torch.float32: np.float32, torch.float64: np.float64}


def _fill_word(f, value):
    a = np.zeros(1, dtype=_NP_OF[f.dtype])
    a[0] = value
    return int(a.view(np.uint64 if f.elem_bytes == 8 else np.uint32)[0])


class _PaddedEpoch(_Epoch):
    """One epoch of a padded loader: :class:`_Epoch`'s order and plan; a batch that fits goes into the loader's static tensors, one that
    does not is an ordinary :class:`Batch` of the unpadded path."""

    def __init__(self, loader, order, shared=None):
        super().__init__(loader, order, shared)
        st = self.st
        self.prec = (_abi.gsn_loader_field * len(st.fields))()
        for r, q, f in zip(self.prec, self.rec, st.fields):
            for name, _ in _abi.gsn_loader_field._fields_:
                setattr(r, name, getattr(q, name))
            t = loader._static[f.name]
            r.flags = q.flags | loader._pad_flag[f.name]
            r.dst_rows = int(t.shape[1] if f.kind == _KIND_EDGE_INDEX else t.shape[0])
            r.dst = t.data_ptr() if r.dst_rows else None
            r.dst_stride = r.dst_rows if f.kind == _KIND_EDGE_INDEX else 0

    def __next__(self):
        b = self.b
        if b >= self.n_batches:
            raise StopIteration
        ld, st, sh = self.loader, self.st, self.loader.shape
        first = b * ld.batch_size
        B = min(ld.batch_size, self.P - first)
        totals = self.totals[:, b]
        n_r = int(totals[st.node_cls])
        e_r = int(totals[st.edge_cls]) if st.edge_cls >= 0 else 0
        if not padded_fits(sh, B, n_r, e_r):
            return super().__next__()
        self.b = b + 1
        pad = _abi.gsn_loader_pad(B, sh.graph_slots, n_r, e_r, sh.node_capacity, sh.edge_capacity, sh.n_chunk, sh.e_chunk)
        out = ld._batch
        has_edges = st.edge_cls >= 0
        with _abi.device_guard(st.device):
            _abi.check(_abi.lib().gsn_loader_collate_padded_hip(len(self.prec), self.prec, ld._fill_words, self.order_ptr, self.plan_ptr, self.stride,
                                                                first, pad, out.batch.data_ptr(), out.ptr.data_ptr(),
                                                                ld._edge_ptr_dev.data_ptr() if has_edges else None, out.n_valid.data_ptr(),
                                                                _abi.current_stream()), "gsn_loader_collate_padded_hip")
        # the tensors were written behind PyTorch's back: whatever is cached per input tensor and version (aggregation index, packs) is stale
        torch.autograd.graph.increment_version(ld._tensors)
        out.num_real_graphs, out.num_real_nodes, out.num_real_edges = B, n_r, e_r
        pn, pe = pad_pointers(sh, B, n_r, e_r)
        node_ptr = np.empty(sh.graph_slots + 1, dtype=np.int64)
        node_ptr[:B] = self.plan[st.node_cls, first:first + B]
        node_ptr[B:] = pn
        out.node_ptr = node_ptr
        if has_edges:
            edge_ptr = np.empty(sh.graph_slots + 1, dtype=np.int64)
            edge_ptr[:B] = self.plan[st.edge_cls, first:first + B]
            edge_ptr[B:] = pe
            out.edge_ptr = edge_ptr
        return out


class PaddedDataLoader(DataLoader):
    """:class:`DataLoader` with every batch collated into ONE set of static tensors of fixed capacity, by one launch
    (``gsn_loader_collate_padded_hip``): ``node_capacity`` vertices, ``edge_capacity`` edge columns and ``graph_slots = batch_size +
    pad_slots`` graphs.  The real graphs come first, laid out exactly as the :class:`DataLoader` batch of the same generator state; the
    slots behind them hold *pad graphs* of 1 .. ``n_chunk`` vertices and 0 .. ``e_chunk`` self-loop columns that use up the capacities
    exactly (:func:`padded_shape`, :func:`pad_pointers`).  Pad rows of per-vertex and per-edge fields are zero (code 0 is valid for every
    encoder), of per-graph fields NaN (floating) or 0 (integer); ``fill={"name": value}`` overrides a field's fill.

    A field is per-vertex when it shares ``x``'s row pointer, per-edge when it shares ``edge_index``'s, per-graph when every graph has one
    row of it (in a dataset of single-vertex graphs, where that is ambiguous: ``y`` and scalar attributes are per-graph, the rest
    per-vertex); any other field (a ``degrees`` cut short) is refused with ``ValueError``.

    UNLIKE a :class:`Batch`, the :class:`PaddedBatch` does not stay valid: every ``next()`` returns the SAME object with the SAME tensors,
    refilled (every byte of them is rewritten by every launch).  That is what lets a step over it be captured into a HIP graph once
    (``evaluation.GraphedEpoch``).  Hence one live iterator per loader: a second ``iter()`` while an unfinished one is alive raises
    ``RuntimeError``.  Default capacities hold every batch; with explicit smaller ones a batch that does not fit is delivered as an
    ordinary unpadded :class:`Batch`.  The models take a padded batch in evaluation mode as it is; in training mode they refuse it (its pad
    rows would enter the BatchNorm statistics) unless the forward runs under :func:`masked_training`, the opt-in under which BatchNorm
    counts the real rows only (``graphs.PaddedTrainStep`` is the training loop over this loader: one collate launch and one graph replay
    per batch)."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, generator=None, node_capacity=None, edge_capacity=None, fill=None):
        super().__init__(dataset, batch_size, shuffle, drop_last, generator)
        ds = self.dataset
        st = ds._st
        fill = dict(fill or {})
        unknown = sorted(set(fill) - set(st.by_name))
        if unknown:
            raise ValueError("PaddedDataLoader: fill names %s, the dataset has %s" % (unknown, ds.field_names))
        self._pad_flag = {}
        for f in st.fields:
            one_row = bool((st.sizes[f.cls][ds._index] == 1).all())
            if f.name == _NODE_FIELD or f.kind == _KIND_EDGE_INDEX:
                flag = 0
            elif f.cls == st.node_cls and not (one_row and (f.scalar or f.name == "y")):
                flag = 0
            elif f.cls == st.edge_cls:
                flag = _F_PAD_EDGES
            elif one_row:
                flag = _F_PAD_GRAPH
            else:
                raise ValueError("PaddedDataLoader: field %r has rows per graph that are neither the vertices, the edge columns nor one: "
                                 "it has no padded layout" % f.name)
            self._pad_flag[f.name] = flag
        n_sizes = ds.host_sizes(_NODE_FIELD)
        e_sizes = ds.host_sizes(_EDGE_FIELD) if st.edge_cls >= 0 else np.zeros_like(n_sizes)
        self.shape = sh = padded_shape(n_sizes, e_sizes, self.batch_size, self.shuffle, self.drop_last, node_capacity, edge_capacity)
        self.node_capacity, self.edge_capacity, self.pad_slots, self.graph_slots = sh.node_capacity, sh.edge_capacity, sh.pad_slots, sh.graph_slots
        dev = st.device
        batch = PaddedBatch()
        batch._device = dev
        self._static = {}
        self._fill_words = (ctypes.c_uint64 * len(st.fields))()
        for j, f in enumerate(st.fields):
            flag = self._pad_flag[f.name]
            if f.kind == _KIND_EDGE_INDEX:
                t = torch.zeros((2, sh.edge_capacity), dtype=torch.int64, device=dev)
            else:
                rows = sh.graph_slots if flag == _F_PAD_GRAPH else sh.edge_capacity if flag == _F_PAD_EDGES else sh.node_capacity
                t = torch.zeros((rows,) + (() if f.scalar else f.trailing), dtype=f.dtype, device=dev)
                default = float("nan") if flag == _F_PAD_GRAPH and f.dtype.is_floating_point else 0
                self._fill_words[j] = _fill_word(f, fill.get(f.name, default))
            self._static[f.name] = t
            setattr(batch, f.name, t)
        batch.batch = torch.zeros((sh.node_capacity,), dtype=torch.int64, device=dev)
        ptrs = torch.zeros((2, sh.graph_slots + 1), dtype=torch.int64, device=dev)
        batch.ptr, self._edge_ptr_dev = ptrs[0], ptrs[1]
        batch.num_graphs = sh.graph_slots
        batch.n_valid = torch.zeros((1,), dtype=torch.int64, device=dev)
        batch.num_real_graphs = batch.num_real_nodes = batch.num_real_edges = 0
        if st.edge_cls >= 0:
            batch.graph_partition = (batch.ptr, self._edge_ptr_dev, sh.n_chunk, sh.e_chunk, False)
        self._batch = batch
        self._tensors = list(self._static.values()) + [batch.batch, ptrs, batch.n_valid]
        self._live = None
        self.graphed_epochs = {}          # evaluation.test / test_ogb keep their GraphedEpoch per (model, loss, metric) here

    def static_tensors(self):
        """Every device tensor a padded batch is made of (fields, ``batch``, the two pointers in one [2, G_cap + 1] tensor, ``n_valid``)."""
        return list(self._tensors)

    def __iter__(self):
        live = self._live() if self._live is not None else None
        if live is not None and live.b < live.n_batches:
            raise RuntimeError("PaddedDataLoader: an unfinished iterator of this loader is alive, and there is one set of static tensors "
                               "(its batch would be overwritten)")
        perm = self._order.draw(len(self.dataset))
        self.last_permutation = perm
        ep = _PaddedEpoch(self, perm.numpy(), None if self.shuffle else self._sequential)
        if not self.shuffle:
            self._sequential = ep.shared
        self._live = weakref.ref(ep)
        return ep
