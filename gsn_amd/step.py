"""HP-1 + HP-2 of a collated batch as ONE host call and TWO kernel launches (``gsn_count_layer_step_hip``).

What the reference reaches in three Python-level stages -- ``subgraph_counts2ids`` (utils_ids.py:7-29: the int64 identifiers), the
one-hot encoders on ``data.x`` / ``data.edge_features`` / ``data.identifiers`` (utils_graph_learning.py:170-187, called from
models_graph_classification.py:204-222) and ``GSN_edge_sparse.forward`` of layer 0 (GSN_edge_sparse.py:82-170, which re-sorts the
edges into a sparse tensor, :136-139) -- runs here as

* the counting kernel, whose workgroups also leave the target-sorted CSR of their graph, the node pack (one-hot of the atom codes) and
  the whole edge pack rows (identifier classes + one-hot of the bond codes): ``gsn_count_encode_pack16_side_hip``;
* the one-launch layer on those packs: ``gsn_layer_fused_fwd_pack16_hip``.

Layer 0's inputs are one-hot encodings of a few integer codes, so the step does not write them out as rows at all where it need not
(``gsn_count_layer_step_keys_hip``): the counting launch leaves one key byte per vertex, one key word per sorted column and a 16-bit mask of
the identifier classes per column, and the layer gathers its operand rows from a node DICTIONARY (one row per code tuple, built once by
``gsn_one_hot_pack16_hip`` itself) and a byte table -- the same fragments bit for bit, ~0.2 GB per 65 536 molecules neither written nor
read back.  The key path is taken when the dictionary has at most 256 rows (``keys_path_ok``); otherwise the packs, as before.  With at
most 31 rows (``tables_path_ok``) the edge stage does not multiply the x_i chunks either: its accumulators start from a table of that product
per dictionary row, made once per prepared weight set by the kernel's own instructions (``gsn_layer_key_tables_hip``) -- the same bits.

``CountLayerStep`` keeps the two argument structs of the C entry filled in, so a step costs one foreign call (the eager composition
``count_batch`` + ``layer(Codes, ...)`` costs six launches through ~0.3 ms of Python).  Results are those of the composition, bit for bit
(``tests/test_step_gpu.py``).  There is no fallback: a layer / plan the two kernels do not take raises at construction.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _abi, _dense, flags, packs
from ._index import Codes, _CSR


def node_key_radices(n_classes, clamp):
    """Digits per node code column of the dictionary key: the column's classes, plus the digit "none" (a code outside them) without clamp."""
    return [int(c) + (0 if clamp else 1) for c in n_classes]


def node_key(codes, n_classes, clamp):
    """Row of each code tuple in the node dictionary: the mixed-radix number of its digits, column 0 most significant (``codes`` integer
    array / tensor [R, C]; works on numpy arrays and torch tensors alike)."""
    key = 0
    for c, (ncls, radix) in enumerate(zip(n_classes, node_key_radices(n_classes, clamp))):
        x = codes[:, c]
        if clamp:
            x = x.clip(0, ncls - 1)
        digit = x * ((x >= 0) & (x < ncls)) + ncls * ((x < 0) | (x >= ncls))
        key = key * radix + digit
    return key


def node_dict_tuples(n_classes, clamp):
    """The dictionary's code tuples int64 [rows, C], row k = the tuple whose ``node_key`` is k (the digit "none" as the code n_classes[c], which
    the unclamped encoder leaves as a zero segment)."""
    radices = node_key_radices(n_classes, clamp)
    grids = np.meshgrid(*[np.arange(r, dtype=np.int64) for r in radices], indexing="ij")
    return np.stack([g.reshape(-1) for g in grids], axis=1)


def keys_path_ok(n_classes, clamp):
    """The gate of the key path: one byte names a dictionary row."""
    return int(np.prod(node_key_radices(n_classes, clamp), dtype=np.int64)) <= 256


TABLE_ROWS = 31        # rows of the layer kernel's x_i tables (gsn_layer_key_tables_max_rows): what fits the room of the fragments they replace


def tables_path_ok(n_classes, clamp):
    """The gate of the table arm of the key path (``gsn_count_layer_step_tabs_hip``): the node dictionary has at most TABLE_ROWS rows.  The
    tables hold the edge stage's accumulators behind the x_i chunks, which depend on the target's dictionary row alone whatever the weights
    are, so no property of the weights enters (a table for node stage 0's [x | deg] chunks would need the folded weight's degree column
    W3a b2 to be zero, which it is not for a msg_fn with a bias: no such table is built)."""
    return keys_path_ok(n_classes, clamp) and int(np.prod(node_key_radices(n_classes, clamp), dtype=np.int64)) <= TABLE_ROWS


def _tables_switch():
    """GSN_RP_TABLES (csrc/switches.h; read at every step): 0 keeps the layer on its KEYS arm."""
    v = os.environ.get("GSN_RP_TABLES")
    if v is None:
        return True
    try:
        return int(v) != 0
    except ValueError:
        return False


_NODE_DICTS = {}


def node_dictionary(n_classes, clamp, dev):
    """fp16 [rows, 32] on ``dev``: row k = what gsn_one_hot_pack16_hip(col0 = 0, one_col = 31) writes for tuple k (built by that very call)."""
    key = (tuple(int(c) for c in n_classes), bool(clamp), str(dev))
    d = _NODE_DICTS.get(key)
    if d is None:
        tuples = torch.from_numpy(node_dict_tuples(n_classes, clamp)).to(dev)
        d = torch.empty((tuples.shape[0], packs.NODE_COLS), dtype=torch.float16, device=dev)
        ncls = np.asarray(key[0], dtype=np.int32)
        st = torch.zeros(1, dtype=torch.int32, device=dev)      # (the "none" digits are out of range on purpose)
        with _abi.device_guard(dev):
            _abi.check(_abi.lib().gsn_one_hot_pack16_hip(tuples.shape[0], tuples.shape[1], tuples.data_ptr(), _abi.ptr(ncls), 0, d.data_ptr(),
                                                         packs.NODE_COLS, 0, packs.NODE_COLS - 1, st.data_ptr(), _abi.current_stream()), "gsn_one_hot_pack16_hip")
        if torch.cuda.is_current_stream_capturing():      # (recorded with the capture: built again by every replay, not kept here)
            return d
        torch.cuda.current_stream(dev).synchronize()
        _NODE_DICTS[key] = d
    return d


class _StepBuffers(dict):
    """The batch-shaped device buffers of a step.  On the key path no pack is stored: ``["npack"]`` / ``["epack"]`` are then expanded from the
    keys the last step wrote, each time they are asked for (``CountLayerStep.packs``)."""
    expand = None

    def __missing__(self, name):
        if name in ("npack", "epack") and self.expand is not None:
            return self.expand()[0 if name == "npack" else 1]
        raise KeyError(name)


class CountLayerStep:
    """``step = CountLayerStep(plan, layer, id_classes)``; ``ids, y, status = step(node_ptr, edge_ptr, edge_index, x_codes, ef_codes,
    max_nodes, max_edges)``.

    plan        edge-mode :class:`gsn_amd.counting.CountPlan` (GSN-e identifiers)
    layer       a ``GSN_edge_sparse`` with msg_kind='general', id_scope='local', two-stage msg_fn, every width 128, in eval mode
                (the shapes of ``gsn_layer_fused_pack16_supported``)
    id_classes  classes per identifier column of the one-hot encoder (counts above the last class are clamped to it when ``clamp``)
    x_codes / ef_codes   :class:`gsn_amd.layers.Codes` (int64 codes + class counts) of the batch's vertices / columns
    Returns the int64 identifiers [E, plan.n_cols], the layer output fp32 [N, d_out] and the per-graph status words (device, not read)."""

    def __init__(self, plan, layer, id_classes, clamp=True, force_packs=False):
        if plan.mode != "edge":
            raise ValueError("CountLayerStep: an edge-mode plan (GSN-e identifiers)")
        if getattr(plan, "wide", False):
            raise ValueError("CountLayerStep: wide plans count only (patterns of at most 9 vertices here)")
        self.plan, self.layer = plan, layer
        self.id_classes = [int(c) for c in id_classes]
        if len(self.id_classes) != plan.n_cols or min(self.id_classes) < 1:
            raise ValueError("CountLayerStep: one class count >= 1 per identifier column (%d columns)" % plan.n_cols)
        self.clamp = bool(clamp)
        self._enc_tab = np.asarray(self.id_classes, dtype=np.int32)
        if not (layer._one_launch_shape() and layer.has_ids):      # (with identifiers, and those per edge: the counting kernel's GSN-e rows)
            raise ValueError("CountLayerStep: a `general` GSN_edge_sparse layer with id_scope='local' and a two-stage msg_fn")
        self._bufs = None          # (key, dict) of the batch-shaped device buffers
        self._lay = None           # (key, structs) of the layer call
        self._count_call = _abi.gsn_count_call()
        self._side = _abi.gsn_count_side()
        self._layer_call = _abi.gsn_layer_pack16_call()
        self._pk = _abi.gsn_pack16()
        self._keys = _abi.gsn_count_keys()
        self._force_packs = bool(force_packs)      # (tests: the pack path on shapes the key path takes)
        self.on_keys = False                       # which path the last step took
        self.on_tables = False                     # ... and whether its edge stage started from the x_i tables (tables_path_ok)
        self._dict = None
        self._bound = None

    # ---- buffers and structs ----------------------------------------------------------------------------------------------
    def _buffers(self, N, E, G, dev, keys):
        key = (N, E, G, str(dev), keys)
        if self._bufs is None or self._bufs[0] != key:
            b = _StepBuffers()
            b.update({
                "seg_ptr": torch.empty(N + 1, dtype=torch.int32, device=dev), "perm": torch.empty(max(E, 1), dtype=torch.int32, device=dev),
                "tgt": torch.empty(max(E, 1), dtype=torch.int32, device=dev), "src": torch.empty(max(E, 1), dtype=torch.int32, device=dev),
                "status": torch.empty(max(G, 1), dtype=torch.int32, device=dev), "code_status": torch.zeros(1, dtype=torch.int32, device=dev),
            })
            if keys:
                b.expand = self.packs
                # the compact outputs (every entry written by the launch): key byte per vertex, key word per sorted column, identifier mask per column
                b["nkey"] = torch.empty(N, dtype=torch.uint8, device=dev)
                b["ekeys"] = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
                b["idmask"] = torch.empty(max(E, 1), dtype=torch.int16, device=dev)
            else:
                # (every row of both packs is written whole by the counting workgroups: no zero fill)
                b["npack"] = torch.empty((N, packs.NODE_COLS), dtype=torch.float16, device=dev)
                b["epack"] = torch.empty((max(E, 1), packs.EDGE_COLS), dtype=torch.float16, device=dev)
            self._bufs = (key, b)
            self._lay = None
            self._bound = None
        return self._bufs[1]

    def _layer_structs(self, b, N, E, d_x, w_e):
        """The stage descriptors / prepared weights of the layer call (rebuilt when a parameter or a BatchNorm buffer moved)."""
        layer = self.layer
        if layer.training:
            raise RuntimeError("CountLayerStep: the layer must be in eval mode (train-mode BatchNorm takes batch statistics: not this kernel)")
        mf, uf = layer.msg_fn, layer.update_fn
        w_first = layer._folded_first_weight(d_x)
        dev = b["seg_ptr"].device
        sb = [(torch.empty((0, d_x), dtype=torch.float32, device=dev), None)]   # (only for mlp.stages' width bookkeeping)
        edge_stages = mf.stages(sb, upto=len(mf.fc) - 1)
        node_stages = uf.stages(sb, first_weight=w_first, post=None)
        stages = edge_stages + node_stages
        for st in stages:
            if st.act not in ("identity", "relu"):
                raise ValueError("CountLayerStep: activation %r is outside the one-launch layer kernel" % st.act)
            if st.bn is not None and (st.bn.training or st.bn.running_mean is None):
                raise RuntimeError("CountLayerStep: a BatchNorm1d in train mode / without running statistics")
        key = (tuple(_dense._prep_key(st) for st in stages), d_x, getattr(layer, "_fold_gen", 0), N, E, self.on_keys, 0 if self._dict is None else self._dict.data_ptr(),
               self.on_tables)
        if self._lay is not None and self._lay[0] == key:
            return self._lay[1]
        for st in stages:
            st.bn_params, st.bn_invstd = _dense._bn_eval_vectors(st.bn)
        keep = []
        # the edge stage's blocks: x through the sorted targets, x through the sorted sources, the edge pack's columns through perm -- their rows
        # are the two packs (empty fp32 placeholders give the widths)
        ew = torch.empty((0, w_e), dtype=torch.float32, device=dev)
        ge = _dense._stage_struct(edge_stages[0], [(sb[0][0], b["tgt"]), (sb[0][0], b["src"]), (ew, b["perm"])], keep)
        for i in range(3):       # (on keys: the node rows are the dictionary's; the third pointer is not read)
            if self.on_keys:
                ge.blocks[i].data = self._dict.data_ptr() if i < 2 else b["idmask"].data_ptr()
            else:
                ge.blocks[i].data = b["npack"].data_ptr() if i < 2 else b["epack"].data_ptr()
        g0 = _dense._stage_struct(node_stages[0], [], keep)
        g1 = _dense._stage_struct(node_stages[1], [], keep)
        L = _abi.lib()
        if node_stages[0].weight.shape[1] != d_x + edge_stages[0].weight.shape[0] + 4 or edge_stages[0].weight.shape[1] != 2 * d_x + w_e:
            raise ValueError("CountLayerStep: the layer's widths do not match the codes (d_x %d, edge-level columns %d)" % (d_x, w_e))
        if not L.gsn_layer_fused_pack16_supported(ctypes.byref(ge), d_x, ctypes.byref(g0), ctypes.byref(g1)):
            raise ValueError("CountLayerStep: shape outside the packed-row layer kernel (every stage 128 wide, d_x + 4 <= 32, <= 16 edge-level columns)")
        prep = _dense._prepared("_pack16", ge, g0, g1, d_x, dev)
        tabs = None
        if self.on_tables:
            # the x_i tables belong to this prepared buffer and this dictionary: made with it (under capture: recorded with it)
            tabs = torch.empty(int(L.gsn_layer_key_tables_words()), dtype=torch.float32, device=dev)
            with _abi.device_guard(dev):
                _abi.check(L.gsn_layer_key_tables_hip(prep.data_ptr(), self._dict.data_ptr(), self._dict.shape[0], tabs.data_ptr(), _abi.current_stream()),
                           "gsn_layer_key_tables_hip")
        d_out = node_stages[1].weight.shape[0]
        flops = 2.0 * E * edge_stages[0].weight.shape[1] * edge_stages[0].weight.shape[0]
        flops += 2.0 * N * (node_stages[0].weight.shape[1] * node_stages[0].weight.shape[0] + node_stages[1].weight.shape[1] * d_out)
        val = (ge, g0, g1, prep, keep, d_out, flops, tabs)
        self._lay = (key, val)
        self._bound = None
        return val

    # ---- the step ---------------------------------------------------------------------------------------------------------
    def __call__(self, node_ptr, edge_ptr, edge_index, x_codes, ef_codes, max_nodes, max_edges, ids_out=None, ids_are_global=True, out=None):
        _abi.require_gpu()
        if not (isinstance(x_codes, Codes) and isinstance(ef_codes, Codes)):
            raise TypeError("CountLayerStep: x_codes / ef_codes are gsn_amd.layers.Codes (integer codes + class counts)")
        dev = edge_index.device
        N, E, G = x_codes.codes.shape[0], edge_index.shape[1], node_ptr.numel() - 1
        if ef_codes.codes.shape[0] != E or edge_index.dtype != torch.int64 or edge_index.shape[0] != 2 or edge_index.stride(1) != 1:
            raise ValueError("CountLayerStep: edge_index int64 [2, E] with unit column stride, one edge code row per column")
        if E == 0 or G == 0:
            raise ValueError("CountLayerStep: an edge-less batch has no GSN-e identifiers (use the layer's own forward)")
        d_x, w_ids, w_ef = sum(x_codes.n_classes), sum(self.id_classes), sum(ef_codes.n_classes)
        if d_x > packs.NODE_COLS - 4 or w_ids + w_ef > packs.EDGE_COLS or len(x_codes.n_classes) > 4 or len(ef_codes.n_classes) > 4 or w_ids % 4 or w_ef > 8:
            raise ValueError("CountLayerStep: code widths outside the packs (node %d <= 28, edge %d + %d <= 16, identifier classes a multiple of 4, "
                             "<= 8 edge code classes)" % (d_x, w_ids, w_ef))
        keys = not self._force_packs and keys_path_ok(x_codes.n_classes, x_codes.clamp)
        self.on_keys = keys
        self.on_tables = keys and tables_path_ok(x_codes.n_classes, x_codes.clamp) and _tables_switch()
        self._dict = node_dictionary(x_codes.n_classes, x_codes.clamp, dev) if keys else None
        b = self._buffers(N, E, G, dev, keys)
        ge, g0, g1, prep, _keep, d_out, flops, tabs = self._layer_structs(b, N, E, d_x, w_ids + w_ef)
        if ids_out is None:
            ids_out = torch.empty((E, self.plan.n_cols), dtype=torch.int64, device=dev)
        y = out if out is not None else torch.empty((N, d_out), dtype=torch.float32, device=dev)
        c, s, l = self._count_call, self._side, self._layer_call
        bound = (node_ptr.data_ptr(), edge_ptr.data_ptr(), edge_index.data_ptr(), edge_index.stride(0), x_codes.codes.data_ptr(), ef_codes.codes.data_ptr(),
                 int(max_nodes), int(max_edges), bool(ids_are_global), tuple(x_codes.n_classes), tuple(ef_codes.n_classes), x_codes.clamp, ef_codes.clamp, id(prep),
                 keys)
        if self._bound != bound:
            tab = self.plan.device_table(dev)
            c.plan_host = _abi.ptr(self.plan.table); c.plan_dev = tab.data_ptr(); c.plan_words = len(self.plan.table); c.n_graphs = G
            c.node_ptr = node_ptr.data_ptr(); c.edge_ptr = edge_ptr.data_ptr(); c.edge_index = edge_index.data_ptr(); c.edge_row_stride = edge_index.stride(0)
            c.ids_are_global = int(bool(ids_are_global)); c.max_nodes = int(max_nodes); c.max_edges = int(max_edges)
            c.status = b["status"].data_ptr(); c.n_classes = _abi.ptr(self._enc_tab); c.clamp = int(self.clamp)
            c.pack = 0 if keys else b["epack"].data_ptr(); c.pack_stride = packs.EDGE_COLS; c.pack_col0 = 0
            s.csr_row = self.layer._sel(); s.seg_ptr = b["seg_ptr"].data_ptr(); s.perm = b["perm"].data_ptr()
            s.sorted_target = b["tgt"].data_ptr(); s.sorted_other = b["src"].data_ptr(); s.n_nodes = N; s.n_edges = E
            s.node_codes = x_codes.codes.data_ptr(); s.node_code_cols = len(x_codes.n_classes); s.node_clamp = int(x_codes.clamp)
            s.edge_codes = ef_codes.codes.data_ptr(); s.edge_code_cols = len(ef_codes.n_classes); s.edge_clamp = int(ef_codes.clamp)
            for i in range(4):
                s.node_n_classes[i] = x_codes.n_classes[i] if i < len(x_codes.n_classes) else 0
                s.edge_n_classes[i] = ef_codes.n_classes[i] if i < len(ef_codes.n_classes) else 0
            s.node_pack = 0 if keys else b["npack"].data_ptr(); s.edge_col0 = w_ids; s.code_status = b["code_status"].data_ptr()
            c.side = ctypes.pointer(s)
            if keys:
                k = self._keys
                k.nkey = b["nkey"].data_ptr(); k.ekeys = b["ekeys"].data_ptr(); k.idmask = b["idmask"].data_ptr()
                self._pk.node_rows = 0; self._pk.edge_rows = 0
            else:
                self._pk.node_rows = b["npack"].data_ptr(); self._pk.edge_rows = b["epack"].data_ptr()
            l.n_nodes = N; l.n_edges = E; l.seg_ptr = b["seg_ptr"].data_ptr(); l.edge = ctypes.pointer(ge); l.d_x = d_x
            l.x = self._dict.data_ptr() if keys else b["npack"].data_ptr()
            l.node0 = ctypes.pointer(g0); l.node1 = ctypes.pointer(g1); l.prepared = prep.data_ptr(); l.pack = ctypes.pointer(self._pk); l.edge_rows = E
            self._bound = bound
        c.out = ids_out.data_ptr()
        l.out = y.data_ptr()
        timer = flags.KERNEL_TIMER
        L = _abi.lib()
        if keys:
            kref, dptr, drows = ctypes.byref(self._keys), self._dict.data_ptr(), self._dict.shape[0]
            entry = "gsn_count_layer_step_tabs_hip"
            tptr = tabs.data_ptr() if tabs is not None else None

            def call(ev_between):
                return L.gsn_count_layer_step_tabs_hip(ctypes.byref(c), ctypes.byref(l), kref, dptr, drows, tptr, ev_between, _abi.current_stream())
        else:
            entry = "gsn_count_layer_step_hip"

            def call(ev_between):
                return L.gsn_count_layer_step_hip(ctypes.byref(c), ctypes.byref(l), ev_between, _abi.current_stream())
        if timer is None:
            with _abi.device_guard(dev):
                rc = call(None)
        else:
            # measuring host (bench.py): HIP events around the two kernels of the one call -- the middle one is recorded by the library between its
            # two launches; entries under the names the separate launches use ("count", "layer_fused")
            only = flags.KERNEL_TIMER_ONLY
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            with _abi.device_guard(dev):
                ev[1].record()                         # (creates the handle the library records again below)
                if only is None or "count" in only:
                    ev[0].record()
                rc = call(ev[1].cuda_event)
                ev[2].record()
            if only is None or "count" in only:
                # bytes of the counting launch: edge_index, int64 identifiers, the identifier columns of the pack (keys: a 2-byte mask); side
                # workgroups: edge_index and codes in, node pack (keys: a byte), edge-code columns (keys: the 4-byte key word), CSR arrays out
                if keys:
                    nbytes = 16.0 * E + 8.0 * E * self.plan.n_cols + 2.0 * E + 16.0 * E + 9.0 * N + 12.0 * E + 12.0 * E + 4.0 * N
                else:
                    nbytes = 16.0 * E + 8.0 * E * self.plan.n_cols + 2.0 * E * w_ids + 16.0 * E + 72.0 * N + 16.0 * E + 12.0 * E + 4.0 * N
                timer.setdefault("count", []).append((ev[0], ev[1], nbytes))
            if only is None or "layer_fused" in only:
                timer.setdefault("layer_fused", []).append((ev[1], ev[2], flops))
        _abi.check(rc, entry)
        self._last = (w_ids, d_x)
        return ids_out, y, b["status"]

    def csr(self):
        """The CSR arrays the last step wrote (seg_ptr, perm, sorted targets, sorted sources) as a layers-side _CSR object."""
        b = self._bufs[1]
        c = _CSR()
        c.seg_ptr, c.perm, c.tgt, c.src, c.part = b["seg_ptr"], b["perm"], b["tgt"], b["src"], None
        c._deg = c._deg4 = None
        return c

    def packs(self):
        """(node pack, edge pack) of the last step: what it wrote, or on the key path the expansion of what it wrote -- the key bytes through
        the dictionary, the identifier masks plus the edge-code bits of the key words scattered back through perm.  Never re-encoded from
        the input codes: these are the data the layer consumed."""
        b = self._bufs[1]
        if "npack" in b:
            return b["npack"], b["epack"]
        w_ids = self._last[0]
        npack = self._dict[b["nkey"].long()]
        bond = torch.zeros_like(b["ekeys"])
        bond[b["perm"].long()] = (b["ekeys"] >> 16) & 0xff          # (sorted order -> column order)
        mask = (b["idmask"].to(torch.int32) & 0xffff) | (bond << w_ids)
        cols = torch.arange(packs.EDGE_COLS, dtype=torch.int32, device=mask.device)
        epack = ((mask.unsqueeze(1) >> cols.unsqueeze(0)) & 1).to(torch.float16)
        return npack, epack

    def check_status(self):
        """Read the status words of the last step back (a host synchronisation) and raise the reference's errors."""
        from .counting import _raise_statuses
        b = self._bufs[1]
        _raise_statuses(b["status"])
        if int(b["code_status"].item()) != 0:
            raise IndexError("a code outside its column's classes (one-hot encoding of integer codes)")
