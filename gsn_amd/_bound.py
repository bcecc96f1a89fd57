"""Row bounds of a padded batch in training mode.

A padded batch (loader.PaddedBatch) keeps its real rows in front: vertices ``[0, N_r)``, edge columns ``[0, E_r)``, graphs ``[0, b)``.  A
``RowBound`` names one of those prefixes by what the collate launch left ON THE DEVICE -- ``n_valid`` (int64 [1]) and optionally a pointer
tensor ``row_ptr`` (int64 [n_slots + 1]) indexed by it -- so that the train-mode BatchNorm kernels take their statistics over the real rows
only, under eager execution and under the replay of a captured step alike.  ``host_rows`` is the same count on the host, for checks that
can only be made eagerly (a single real row is refused as torch refuses it).

``masked_training(batch)`` installs the three bounds of a batch (row classes ``"vertex"``, ``"edge"``, ``"graph"``) for the length of a
``with`` block; under it the models accept the padded batch in training mode, every train-mode BatchNorm stage asks for the bound of the
row class its CALL SITE names (never inferred from a row count: the capacities may be equal), and a statistics path that was not given one
raises ``RuntimeError`` naming itself."""
from __future__ import annotations

import contextlib

import torch

ROW_CLASSES = ("vertex", "edge", "graph")


class RowBound:
    """``v = clamp(row_ptr[clamp(n_valid, 0, n_slots)] if row_ptr is not None else n_valid, 0, m_rows)``, evaluated by the kernels."""
    __slots__ = ("n_valid", "row_ptr", "n_slots", "host_rows", "used")

    def __init__(self, n_valid, row_ptr=None, host_rows=None):
        if not isinstance(n_valid, torch.Tensor) or n_valid.dtype != torch.int64 or n_valid.numel() != 1 or not n_valid.is_cuda:
            raise TypeError("RowBound: n_valid is an int64 tensor of one element on the GPU")
        if row_ptr is not None:
            if (not isinstance(row_ptr, torch.Tensor) or row_ptr.dtype != torch.int64 or row_ptr.dim() != 1 or row_ptr.numel() < 1
                    or not row_ptr.is_contiguous()):
                raise TypeError("RowBound: row_ptr is a contiguous 1-D int64 tensor of n_slots + 1 entries")
            if row_ptr.device != n_valid.device:
                raise TypeError("RowBound: row_ptr lives on %s, n_valid on %s" % (row_ptr.device, n_valid.device))
        if host_rows is not None and (isinstance(host_rows, bool) or not isinstance(host_rows, int) or host_rows < 0):
            raise TypeError("RowBound: host_rows = %r (a non-negative int, or None)" % (host_rows,))
        self.n_valid, self.row_ptr, self.host_rows = n_valid, row_ptr, host_rows
        self.n_slots = 0 if row_ptr is None else int(row_ptr.numel()) - 1
        self.used = 0                    # width of a train-mode BatchNorm stage that took its statistics under this bound (0: none did)

    def pointers(self):
        """``(n_valid pointer, row_ptr pointer or None, n_slots)`` as the bounded entries take them"""
        return self.n_valid.data_ptr(), None if self.row_ptr is None else self.row_ptr.data_ptr(), self.n_slots

    def __repr__(self):
        return "RowBound(n_slots=%d, host_rows=%r)" % (self.n_slots, self.host_rows)


_ACTIVE = None          # {row class: RowBound} while a masked_training block is open


def is_active():
    return _ACTIVE is not None


def active(rows, who):
    """The bound of row class ``rows`` if a masked_training block is open, else None.  ``who`` (the statistics path asking) is named by the
    RuntimeError raised when a block is open and the path was not told its row class."""
    if _ACTIVE is None:
        return None
    if rows is None:
        raise RuntimeError("%s: train-mode BatchNorm statistics under loader.masked_training() on a path that does not name its row class "
                           "(the statistics would run over the pad rows)" % who)
    if rows not in _ACTIVE:
        raise ValueError("%s: row class %r (one of %s)" % (who, rows, ", ".join(ROW_CLASSES)))
    return _ACTIVE[rows]


def refuse(who):
    """A train-mode statistics path that has no bounded form: RuntimeError naming it while a masked_training block is open."""
    if _ACTIVE is not None:
        raise RuntimeError("%s: train-mode BatchNorm statistics have no row-bounded form on this path; it cannot run under "
                           "loader.masked_training()" % who)


def bounds_of(batch):
    """The three bounds of a loader.PaddedBatch from what its collate launch wrote: ``n_valid`` = b, ``ptr[b]`` = N_r, the edge pointer's
    entry b = E_r (``graph_partition[1]``)."""
    if not getattr(batch, "padded", False):
        raise TypeError("masked_training: a loader.PaddedBatch, not %s" % type(batch).__name__)
    part = getattr(batch, "graph_partition", None)
    b, n_r, e_r = int(batch.num_real_graphs), int(batch.num_real_nodes), int(batch.num_real_edges)
    out = {"graph": RowBound(batch.n_valid, None, b), "vertex": RowBound(batch.n_valid, batch.ptr, n_r)}
    if part is not None:
        out["edge"] = RowBound(batch.n_valid, part[1], e_r)
    return out


@contextlib.contextmanager
def masked_training(batch):
    """``with masked_training(batch): loss = loss_fn(model(batch), batch.y, n_valid=batch.n_valid)`` -- the opt-in under which
    GNNSubstructures / GNN_OGB take a padded batch in training mode with BatchNorm statistics over its real rows.  Yields the bounds."""
    global _ACTIVE
    if _ACTIVE is not None:
        raise RuntimeError("masked_training: a block is open already (one padded batch at a time)")
    bounds = bounds_of(batch)
    _ACTIVE = bounds
    try:
        yield bounds
    finally:
        _ACTIVE = None
