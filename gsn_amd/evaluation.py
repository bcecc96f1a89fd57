"""Evaluation on the device: the evaluation half of the reference's ``train_test_funcs.py`` without its per-batch host reads.

* ``masked_loss(kind, y_hat, y)`` / ``MaskedLoss(kind)`` -- the OGB training loss ``loss_fn(y_hat[is_labeled], y[is_labeled])`` with
  ``is_labeled = (y == y)`` (train_test_funcs.py:98-101) as ONE autograd node over ``gsn_masked_loss_fwd_hip`` / ``_bwd_hip``.  No boolean
  index, so no ``nonzero``, no host read and no data-dependent shape: it can be captured by ``GraphedStep`` / ``GraphedTrainStep``.
* ``EpochAccumulator`` -- one ``gsn_eval_accumulate_hip`` call per batch (loss sums, metric sum, the batch's rows appended behind a device
  cursor); ``result()`` is the epoch's single host read.
* ``Evaluator`` -- ``rocauc`` / ``ap`` / ``acc`` with ogb's ``Evaluator`` interface, ROC-AUC and average precision from the exact integer
  rank statistics of ``gsn_rank_metrics_hip`` (no ogb, no sklearn).
* ``test`` / ``test_ogb`` -- the reference's evaluation loops (train_test_funcs.py:177-259), same signatures and return values.
* ``GraphedEpoch`` -- the same loops over a ``loader.PaddedDataLoader``: the eval forward and the batch's accumulation captured ONCE into
  a HIP graph over the loader's static batch, then one collate launch and one replay per batch.  ``test`` / ``test_ogb`` use it when they
  are handed such a loader.

There is no fallback: a loss or metric object this module cannot name raises ``TypeError``; without a GPU the entries raise.
Out of scope: the ``train()`` loop, checkpointing, wandb, ``test_isomorphism`` (already one ``pdist`` and one host read).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _abi

LOSS_KINDS = {"BCEWithLogitsLoss": 0, "L1Loss": 1, "MSELoss": 2, "CrossEntropyLoss": 3}          # GSN_LOSS_*
METRIC_KINDS = {None: 0, "None": 0, "L1Loss": 1, "MSELoss": 2, "multi_class_accuracy": 3}       # GSN_METRIC_*
ST_ONE_CLASS, ST_NO_POSITIVE, ST_NONFINITE, ST_BAD_LABEL = 1, 2, 4, 8                            # GSN_RANK_*
MAX_ROWS, MAX_COLS = (1 << 31) - 1, 65535
_NO_CAPACITY = 1 << 62          # the capacity handed to the kernel when no rows are kept


def _kind_of(kind):
    if kind not in LOSS_KINDS:
        raise NotImplementedError("loss %r (one of %s)" % (kind, ", ".join(LOSS_KINDS)))
    return LOSS_KINDS[kind]


def _operands(kind, y_hat, y):
    """(y_hat fp32 contiguous, y fp32 of y_hat's element count / int64 [rows], rows, cols) as the entries take them"""
    if not y_hat.is_cuda:
        _abi.require_gpu()
        raise RuntimeError("gsn_amd.evaluation: y_hat must live on the GPU (there is no CPU fallback)")
    if y_hat.dtype != torch.float32:
        raise TypeError("gsn_amd.evaluation: y_hat must be float32, not %s" % y_hat.dtype)
    y_hat = y_hat.contiguous()
    y = y.to(y_hat.device)
    if kind == "CrossEntropyLoss":
        if y_hat.dim() != 2 or (y_hat.shape[0] > 0 and y_hat.shape[1] == 0):
            raise ValueError("CrossEntropyLoss: y_hat [rows, classes] with at least one class")
        if y.dtype.is_floating_point or y.numel() != y_hat.shape[0]:
            raise ValueError("CrossEntropyLoss: one integer target per row of y_hat")
        return y_hat, y.reshape(-1).to(torch.int64).contiguous(), y_hat.shape[0], y_hat.shape[1]
    if y.numel() != y_hat.numel():
        raise ValueError("%s: y has %d elements, y_hat %d" % (kind, y.numel(), y_hat.numel()))
    cols = y_hat.shape[-1] if y_hat.dim() >= 2 else 1
    rows = y_hat.numel() // cols if cols else 0
    return y_hat, y.to(torch.float32).reshape(y_hat.shape).contiguous(), rows, cols


def _scratch(n_bytes, dev):
    return torch.empty(max(int(n_bytes), 8), dtype=torch.uint8, device=dev) if n_bytes > 0 else None


def _check_n_valid(who, n_valid, device=None):
    if not isinstance(n_valid, torch.Tensor) or n_valid.dtype != torch.int64 or n_valid.numel() != 1 or (device is not None and n_valid.device != device):
        raise TypeError("%s: n_valid is an int64 tensor of one element on the device of y_hat" % who)


class _MaskedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, y, kind, n_valid=None):
        _abi.require_gpu()
        k = _kind_of(kind)
        y_hat, y, rows, cols = _operands(kind, y_hat, y)
        dev = y_hat.device
        L = _abi.lib()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.int64, device=dev)
        nb = L.gsn_masked_loss_scratch_bytes(k, rows, cols)
        ws = _scratch(nb, dev)
        if n_valid is not None:
            _check_n_valid("masked_loss", n_valid, dev)
        with _abi.device_guard(dev):
            if n_valid is None:
                _abi.check(L.gsn_masked_loss_fwd_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), loss.data_ptr(), count.data_ptr(), _abi.ptr(ws), nb,
                                                     _abi.current_stream()), "gsn_masked_loss_fwd_hip")
            else:       # (rows behind n_valid are unlabelled whatever they hold: the row count is read on the device)
                _abi.check(L.gsn_masked_loss_fwd_counted_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), n_valid.data_ptr(), loss.data_ptr(),
                                                             count.data_ptr(), _abi.ptr(ws), nb, _abi.current_stream()), "gsn_masked_loss_fwd_counted_hip")
        ctx.n_valid = n_valid
        ctx.save_for_backward(y_hat, y, count)
        ctx.shape = (k, rows, cols)
        ctx.mark_non_differentiable(count)
        ctx.set_materialize_grads(False)          # (no zero fill for the count's gradient: the node is two launches, forward and backward)
        return loss, count

    @staticmethod
    def backward(ctx, grad_loss, _grad_count):
        if grad_loss is None:
            return None, None, None, None
        y_hat, y, count = ctx.saved_tensors
        k, rows, cols = ctx.shape
        grad = torch.empty_like(y_hat)
        g = grad_loss.to(torch.float32).contiguous()
        if rows and cols:
            with _abi.device_guard(y_hat.device):
                if ctx.n_valid is None:
                    _abi.check(_abi.lib().gsn_masked_loss_bwd_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), g.data_ptr(), count.data_ptr(),
                                                                  grad.data_ptr(), _abi.current_stream()), "gsn_masked_loss_bwd_hip")
                else:
                    _abi.check(_abi.lib().gsn_masked_loss_bwd_counted_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), ctx.n_valid.data_ptr(), g.data_ptr(),
                                                                          count.data_ptr(), grad.data_ptr(), _abi.current_stream()),
                               "gsn_masked_loss_bwd_counted_hip")
        return grad, None, None, None


def masked_loss(kind, y_hat, y, return_count=False, n_valid=None):
    """Mean of the ``kind`` loss over the labelled entries (``y`` not NaN; ``y`` is viewed to ``y_hat``'s shape as train_test_funcs.py:98-99
    does), a 0-d fp32 tensor on ``y_hat``'s device, differentiable in ``y_hat``.  ``CrossEntropyLoss``: ``y`` int64 [rows], nothing is
    unlabelled, a target outside the classes gives a NaN loss and a zero gradient row.  No labelled entry: NaN loss, zero gradient.
    ``n_valid`` (int64 device tensor of one element, a padded batch's ``batch.n_valid``): rows from ``clamp(n_valid, 0, rows)`` on are
    unlabelled whatever they hold and get zero gradient rows; the count is read on the device, so the node can be captured and replayed."""
    if n_valid is not None:
        _check_n_valid("masked_loss", n_valid)
    loss, count = _MaskedLossFn.apply(y_hat, y, kind, n_valid)
    return (loss, count) if return_count else loss


class MaskedLoss(nn.Module):
    """``loss_fn(y_hat, y)`` of the reference with unlabelled (NaN) targets left out: ``MaskedLoss('BCEWithLogitsLoss')``."""

    def __init__(self, kind):
        super().__init__()
        _kind_of(kind)
        self.kind = kind

    def forward(self, y_hat, y, n_valid=None):
        return masked_loss(self.kind, y_hat, y, n_valid=n_valid)

    def extra_repr(self):
        return self.kind


def loss_function(name):
    """utils.py:164-175: the loss of ``--loss_fn`` (here with the mask built in; without NaN targets it is torch's loss)."""
    if name not in LOSS_KINDS:
        raise NotImplementedError
    return MaskedLoss(name)


class PredictionFn:
    """The metric of ``--prediction_fn`` (utils.py:177-183): ``fn(y_hat, y)`` returns its sum over the batch as a 0-d device tensor --
    correct arg-max rows (``multi_class_accuracy``), or the fp32 ``reduction='sum'`` of ``L1Loss`` / ``MSELoss``."""

    def __init__(self, name):
        if name not in METRIC_KINDS or METRIC_KINDS[name] == 0:
            raise NotImplementedError
        self.name = name

    def __call__(self, y_hat, y):
        loss = "CrossEntropyLoss" if self.name == "multi_class_accuracy" else self.name
        acc = EpochAccumulator(0, y_hat.shape[-1] if y_hat.dim() >= 2 else 1, 1, loss, self.name, device=y_hat.device, keep_rows=False)
        acc.add(y_hat, y)
        return (acc._i64[2] if self.name == "multi_class_accuracy" else acc._f64[2]).to(torch.float32)


def prediction_function(name):
    """utils.py:177-187: ``'None'`` -> None, an unknown name raises NotImplementedError."""
    if name == "None":
        return None
    return PredictionFn(name)


def _loss_name(loss_fn):
    """The kind of a loss object: a MaskedLoss, a kind name, or one of torch's four losses with default arguments."""
    if isinstance(loss_fn, MaskedLoss):
        return loss_fn.kind
    if isinstance(loss_fn, str):
        _kind_of(loss_fn)
        return loss_fn
    name = type(loss_fn).__name__
    if isinstance(loss_fn, nn.Module) and name in LOSS_KINDS:
        ok = getattr(loss_fn, "reduction", "mean") == "mean" and getattr(loss_fn, "weight", None) is None and getattr(loss_fn, "pos_weight", None) is None
        if name == "CrossEntropyLoss":
            ok = ok and loss_fn.ignore_index == -100 and getattr(loss_fn, "label_smoothing", 0.0) == 0.0
        if ok:
            return name
    raise TypeError("gsn_amd.evaluation: loss %r is none of %s with default arguments (there is no slow path to fall back to)"
                    % (loss_fn, ", ".join(LOSS_KINDS)))


def _metric_name(prediction_fn):
    if prediction_fn is None:
        return None
    if isinstance(prediction_fn, PredictionFn):
        return prediction_fn.name
    if isinstance(prediction_fn, str) and prediction_fn in METRIC_KINDS:
        return None if prediction_fn == "None" else prediction_fn
    if getattr(prediction_fn, "__name__", None) == "multi_class_accuracy":
        return "multi_class_accuracy"
    name = type(prediction_fn).__name__
    if isinstance(prediction_fn, nn.Module) and name in ("L1Loss", "MSELoss") and prediction_fn.reduction == "sum":
        return name
    raise TypeError("gsn_amd.evaluation: metric %r is none of multi_class_accuracy, L1Loss(reduction='sum'), MSELoss(reduction='sum')" % (prediction_fn,))


class EpochResult:
    """What ``EpochAccumulator.result()`` read: ``weighted_loss_sum`` (sum of loss_b * num_graphs_b), ``batch_loss_sum``, ``n_batches``,
    ``metric_sum``, ``n_rows`` and the device views ``y_pred[:n_rows]`` / ``y_true[:n_rows]`` (None when no rows are kept)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class EpochAccumulator:
    """The sums and rows of one evaluation epoch, kept on the device.

    ``capacity`` rows of ``n_pred_cols`` predictions and ``n_target_cols`` targets (fp32; int64 [capacity, 1] for ``CrossEntropyLoss``);
    ``loss``: a kind name or a loss object; ``metric``: None, ``'L1Loss'``, ``'MSELoss'`` or ``'multi_class_accuracy'`` (with integer
    targets).  ``add`` is one foreign call and reads nothing back; it may be captured (``GraphedStep``): the row cursor lives on the device,
    so every replay appends the refilled batch.  ``result()`` makes the single host read and raises when a batch did not fit."""

    def __init__(self, capacity, n_pred_cols, n_target_cols, loss, metric=None, device=None, keep_rows=True):
        self.loss = _loss_name(loss)
        self.metric = _metric_name(metric)
        self.kind, self.metric_kind = LOSS_KINDS[self.loss], METRIC_KINDS[self.metric]
        if (self.metric_kind == 3) != (self.kind == 3) and self.metric_kind != 0:
            raise ValueError("EpochAccumulator: multi_class_accuracy goes with CrossEntropyLoss (integer targets), the L1 / MSE sums with the other losses")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            _abi.require_gpu()
            raise RuntimeError("EpochAccumulator: a GPU device (there is no CPU fallback)")
        self.device, self.capacity = dev, int(capacity)
        self.n_pred_cols = int(n_pred_cols)
        self.n_target_cols = 1 if self.kind == 3 else int(n_target_cols)
        if self.capacity < 0 or self.capacity > MAX_ROWS:
            raise ValueError("EpochAccumulator: capacity of 0 .. 2^31 - 1 rows")
        self._state = torch.zeros(8, dtype=torch.int64, device=dev)          # one small record: the epoch's single copy
        self._f64 = self._state[:4].view(torch.float64)
        self._i64 = self._state[4:]
        self.keep_rows = bool(keep_rows)
        self.y_pred = self.y_true = None
        if self.keep_rows:
            self.y_pred = torch.empty((self.capacity, self.n_pred_cols), dtype=torch.float32, device=dev)
            self.y_true = torch.empty((self.capacity, self.n_target_cols), dtype=torch.int64 if self.kind == 3 else torch.float32, device=dev)
        self.last_loss = torch.zeros((), dtype=torch.float32, device=dev)      # the loss of the last batch (device)

    def reset(self):
        self._state.zero_()

    def add(self, y_hat, y, num_graphs=None, n_valid=None):
        """One batch.  ``n_valid`` (int64 device tensor of one element): only the first ``clamp(n_valid, 0, rows)`` rows are the batch --
        loss, metric, appended rows, cursor and weight are those of ``add(y_hat[:v], y[:v], v)``, with v read on the device
        (``gsn_eval_accumulate_counted_hip``): the rest of a padded batch is never looked at.  ``num_graphs`` is then not used."""
        _abi.require_gpu()
        y_hat, y, rows, cols = _operands(self.loss, y_hat, y)
        if self.keep_rows and (cols != self.n_pred_cols or (self.kind != 3 and cols != self.n_target_cols)):
            raise ValueError("EpochAccumulator.add: %d prediction columns, buffers of %d / %d" % (cols, self.n_pred_cols, self.n_target_cols))
        L = _abi.lib()
        nb = L.gsn_eval_accumulate_scratch_bytes(self.kind, rows, cols)
        ws = _scratch(nb, self.device)
        if n_valid is not None:
            if not isinstance(n_valid, torch.Tensor) or n_valid.dtype != torch.int64 or n_valid.numel() != 1 or n_valid.device != y_hat.device:
                raise TypeError("EpochAccumulator.add: n_valid is an int64 tensor of one element on the device of y_hat")
            with _abi.device_guard(self.device):
                _abi.check(L.gsn_eval_accumulate_counted_hip(self.kind, self.metric_kind, rows, cols, 1 if self.kind == 3 else cols, y_hat.data_ptr(),
                                                             y.data_ptr(), n_valid.data_ptr(), self._f64.data_ptr(), self._i64.data_ptr(),
                                                             _abi.ptr(self.y_pred), _abi.ptr(self.y_true),
                                                             self.capacity if self.keep_rows else _NO_CAPACITY, self.last_loss.data_ptr(), _abi.ptr(ws), nb,
                                                             _abi.current_stream()), "gsn_eval_accumulate_counted_hip")
            return
        with _abi.device_guard(self.device):
            _abi.check(L.gsn_eval_accumulate_hip(self.kind, self.metric_kind, rows, cols, 1 if self.kind == 3 else cols, y_hat.data_ptr(), y.data_ptr(),
                                                 rows if num_graphs is None else int(num_graphs), self._f64.data_ptr(), self._i64.data_ptr(),
                                                 _abi.ptr(self.y_pred), _abi.ptr(self.y_true), self.capacity if self.keep_rows else _NO_CAPACITY,
                                                 self.last_loss.data_ptr(), _abi.ptr(ws), nb, _abi.current_stream()), "gsn_eval_accumulate_hip")

    def result(self):
        host = self._state.cpu()                                              # the one host read of the epoch
        f64, i64 = host[:4].view(torch.float64), host[4:]
        if int(i64[3]) & 1:
            raise RuntimeError("EpochAccumulator: a batch did not fit into the capacity of %d rows (%d rows held); nothing of it was kept"
                               % (self.capacity, int(i64[0])))
        n = int(i64[0])
        return EpochResult(weighted_loss_sum=float(f64[0]), batch_loss_sum=float(f64[1]), n_batches=int(i64[1]),
                           metric_sum=float(i64[2]) if self.metric_kind == 3 else float(f64[2]), n_rows=n,
                           y_pred=self.y_pred[:n] if self.keep_rows else None, y_true=self.y_true[:n] if self.keep_rows else None)


def rank_metrics(y_pred, y_true):
    """``gsn_rank_metrics_hip`` on device tensors [M, T]: numpy arrays ``(ints [T, 3] = n_labelled, n_pos, U2; floats [T, 2] = auc, ap;
    status [T])`` after ONE host read."""
    _abi.require_gpu()
    if y_pred.dim() != 2 or y_pred.shape != y_true.shape:
        raise RuntimeError("y_true and y_pred must be 2-dim arrays of one shape, (num_graph, num_tasks)")
    m, t = y_pred.shape
    if m > MAX_ROWS or t > MAX_COLS:
        raise ValueError("rank metrics: at most 2^31 - 1 rows and 65535 columns (got %d x %d)" % (m, t))
    dev = y_pred.device
    y_pred = y_pred.to(torch.float32).contiguous()
    y_true = y_true.to(torch.float32).contiguous()
    out = torch.zeros(6 * max(t, 1), dtype=torch.int64, device=dev)
    oi, of, st = out[:3 * t], out[3 * t:5 * t].view(torch.float64), out[5 * t:].view(torch.int32)
    L = _abi.lib()
    nb = L.gsn_rank_metrics_scratch_bytes(m, t)
    ws = _scratch(nb, dev)
    with _abi.device_guard(dev):
        _abi.check(L.gsn_rank_metrics_hip(m, t, y_pred.data_ptr(), y_true.data_ptr(), oi.data_ptr(), of.data_ptr(), st.data_ptr(), _abi.ptr(ws), nb,
                                          _abi.current_stream()), "gsn_rank_metrics_hip")
    host = out.cpu()
    return (host[:3 * t].numpy().reshape(t, 3), host[3 * t:5 * t].view(torch.float64).numpy().reshape(t, 2),
            host[5 * t:].view(torch.int32).numpy()[:t])


_DATASET_METRICS = {"ogbg-molhiv": "rocauc", "ogbg-molpcba": "ap", "ogbg-ppa": "acc"}


class Evaluator:
    """``Evaluator(name).eval({'y_true': ..., 'y_pred': ...})`` -> ``{eval_metric: float}`` as ogb.graphproppred.Evaluator, computed on the
    device.  ``rocauc`` / ``ap``: the mean over the columns that have both classes / a positive (the others are skipped as ogb skips them;
    none left: RuntimeError); a non-finite prediction in a labelled row or a label other than 0, 1, NaN raises ValueError naming the column,
    as sklearn does.  ``acc``: per column the share of equal integer entries among the labelled rows, then the mean over columns.
    Inputs: device tensors, or numpy arrays (uploaded)."""

    def __init__(self, name, eval_metric=None, device=None):
        if eval_metric is None:
            if name not in _DATASET_METRICS:
                raise ValueError("Evaluator: dataset %r is not in the built-in table (%s): spell out eval_metric" % (name, ", ".join(_DATASET_METRICS)))
            eval_metric = _DATASET_METRICS[name]
        if eval_metric not in ("rocauc", "ap", "acc"):
            raise ValueError("Evaluator: eval_metric %r (rocauc, ap or acc)" % (eval_metric,))
        self.name, self.eval_metric, self.device = name, eval_metric, device

    def _tensor(self, a):
        if isinstance(a, torch.Tensor):
            return a if a.is_cuda else a.to(self.device or "cuda")
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device or "cuda")

    def eval(self, input_dict):
        if "y_true" not in input_dict or "y_pred" not in input_dict:
            raise RuntimeError("Missing key of y_true or y_pred")
        _abi.require_gpu()
        y_true, y_pred = self._tensor(input_dict["y_true"]), self._tensor(input_dict["y_pred"])
        if y_true.shape != y_pred.shape or y_true.dim() != 2:
            raise RuntimeError("y_true and y_pred must be 2-dim arrays of one shape, (num_graph, num_tasks)")
        if self.eval_metric == "acc":
            lab = (y_true == y_true)
            share = ((y_true == y_pred) & lab).sum(0).to(torch.float64) / lab.sum(0).to(torch.float64)
            return {"acc": float(share.mean())}
        _ints, floats, status = rank_metrics(y_pred, y_true)
        for c in range(len(status)):
            if status[c] & ST_BAD_LABEL:
                raise ValueError("%s: column %d of y_true holds a label other than 0, 1 or NaN" % (self.eval_metric, c))
            if status[c] & ST_NONFINITE:
                raise ValueError("%s: column %d of y_pred holds NaN or infinity in a labelled row" % (self.eval_metric, c))
        skip = ST_ONE_CLASS if self.eval_metric == "rocauc" else ST_NO_POSITIVE
        vals = [float(floats[c, 0 if self.eval_metric == "rocauc" else 1]) for c in range(len(status)) if not status[c] & skip]
        if not vals:
            raise RuntimeError("No positively labeled data available. Cannot compute %s." % ("ROC-AUC" if self.eval_metric == "rocauc" else "Average Precision"))
        return {self.eval_metric: sum(vals) / len(vals)}


def _batches(loader, n_iters):
    """the reference's iteration: n_iters batches (default: one pass), the loader restarting when it runs out"""
    it = iter(loader)
    n_iters = len(loader) if n_iters is None else n_iters
    for _ in range(n_iters):
        try:
            data = next(it)
        except StopIteration:
            it = iter(loader)
            data = next(it)
        yield data


class GraphedEpoch:
    """An evaluation epoch of ``model`` over a ``loader.PaddedDataLoader`` as one collate launch plus ONE graph replay per batch.

    ``run(n_iters=None)`` returns what ``test(loader, model, loss_fn, device, prediction_fn, n_iters)`` returns -- or, with an
    ``evaluator``, what ``test_ogb(loader, model, loss_fn, device, evaluator, n_iters)`` returns: the same weighting (a batch weighs its
    REAL graphs: the accumulation reads the loader's device-side ``n_valid``), the same single host read at the end, and no branch on
    anything read back from the device.

    On the first padded batch ``model(static_batch)`` followed by ``acc.add(pred, y, n_valid=...)`` is captured through
    ``graphs.GraphedStep`` (``captures`` counts: once per object).  ``layers.invalidate_caches(model)`` runs in front of the captured
    forward, so every derived tensor -- folded weights, eval-mode BatchNorm vectors, transposes, fp16 planes -- is made INSIDE the graph
    from the live parameters and lives in its pool: a replay after optimizer steps, ``load_state_dict`` or anybody's
    ``invalidate_caches`` computes with the parameters as they are then, without version tracking or re-capture.  The price is that every
    replay remakes them.  A batch that did not fit the loader's capacities (an ordinary ``Batch``) runs eagerly into the same accumulator;
    under ``test_ogb``'s rule a batch of one vertex is skipped.  Both are decided from host numbers.  A model in training mode is refused."""

    def __init__(self, model, loader, loss_fn, prediction_fn=None, evaluator=None):
        from .loader import PaddedDataLoader
        if not isinstance(loader, PaddedDataLoader):
            raise TypeError("GraphedEpoch: a loader.PaddedDataLoader (batches of fixed shape in static tensors), not %s" % type(loader).__name__)
        if evaluator is not None and prediction_fn is not None:
            raise ValueError("GraphedEpoch: prediction_fn (the loop of test) or evaluator (the loop of test_ogb), not both")
        self.model, self.loader, self.evaluator = model, loader, evaluator
        self.loss, self.metric = _loss_name(loss_fn), _metric_name(prediction_fn)
        self.ppa = evaluator is not None and evaluator.name == "ogbg-ppa"
        self.acc = self.step = None
        self.captures = self.replays = self.eager_batches = 0

    def _target(self, batch, pred):
        if self.evaluator is None:
            return batch.y
        return batch.y.view(-1) if self.ppa else batch.y.view(pred.shape)

    def _make_acc(self, pred):
        cols = pred.shape[-1] if pred.dim() >= 2 else 1
        if self.evaluator is None:
            self.acc = EpochAccumulator(0, cols, 1, self.loss, self.metric, device=pred.device, keep_rows=False)
        else:      # one pass over the dataset at a time: run() moves the rows out when the loader wraps round
            self.acc = EpochAccumulator(max(len(self.loader.dataset), self.loader.batch_size), pred.shape[1], pred.shape[1], self.loss, None,
                                        device=pred.device)

    def _forward(self, batch):
        from . import layers
        layers.invalidate_caches(self.model)          # (host only: the forward below derives everything from the live parameters)
        pred = self.model(batch)
        if self.acc is None:
            self._make_acc(pred)
        self.acc.add(pred, self._target(batch, pred), n_valid=batch.n_valid)
        return pred

    def _capture(self, batch):
        from . import flags, layers
        from .graphs import GraphedStep
        layers.invalidate_caches(self.model)
        pred = self.model(batch)                      # (eager, with every status check: the first batch's codes are looked at)
        if self.acc is None:
            self._make_acc(pred)
        keep = self.acc._state.clone()                # the warm-up runs are real runs: their sums and rows do not count
        # nothing can be read back inside a capture: the out-of-range flag of the code-gather stages is not looked at under replay (an
        # out-of-range code gives a zero block, as the dense encoder); the eager runs above and below this line do look
        check, flags.CODE_STATUS_CHECK = flags.CODE_STATUS_CHECK, False
        try:
            self.step = GraphedStep(lambda: self._forward(batch), warmup=1, device=self.acc.device)
        finally:
            flags.CODE_STATUS_CHECK = check
        self.acc._state.copy_(keep)
        self.captures += 1

    def run(self, n_iters=None):
        if self.model.training:
            raise RuntimeError("GraphedEpoch: the model is in training mode (padded batches are for model.eval(): their pad rows would enter the "
                               "BatchNorm statistics)")
        ogb = self.evaluator is not None
        held, chunks = 0, []                          # rows behind the accumulator's cursor, counted on the host; rows moved out of it
        if self.acc is not None:
            self.acc.reset()
        with torch.no_grad():
            for batch in _batches(self.loader, n_iters):
                padded = getattr(batch, "padded", False)
                b = batch.num_real_graphs if padded else batch.num_graphs
                if ogb and (batch.num_real_nodes if padded else batch.x.shape[0]) == 1:
                    continue
                if ogb and self.acc is not None and held + b > self.acc.capacity:
                    chunks.append((self.acc.y_pred[:held].clone(), self.acc.y_true[:held].clone()))
                    self.acc._i64[0:1].zero_()
                    held = 0
                if padded:
                    if self.step is None:
                        self._capture(batch)
                    self.step()
                    self.replays += 1
                else:
                    pred = self.model(batch)
                    if self.acc is None:
                        self._make_acc(pred)
                    self.acc.add(pred, self._target(batch, pred), batch.num_graphs)
                    self.eager_batches += 1
                held += b
        n = len(self.loader.dataset)
        if self.acc is None:
            if ogb:
                raise RuntimeError("test_ogb: no batch to evaluate")
            return 0 / n, 0 / n
        r = self.acc.result()
        if not ogb:
            return r.weighted_loss_sum / n, r.metric_sum / n
        y_pred = torch.cat([c[0] for c in chunks] + [r.y_pred]) if chunks else r.y_pred
        y_true = torch.cat([c[1] for c in chunks] + [r.y_true]) if chunks else r.y_true
        if self.ppa:
            y_pred = torch.argmax(y_pred, dim=1).view(-1, 1)
        if not isinstance(self.evaluator, Evaluator):
            y_true, y_pred = y_true.cpu().numpy(), y_pred.cpu().numpy()
        return r.weighted_loss_sum / n, self.evaluator.eval({"y_true": y_true, "y_pred": y_pred})[self.evaluator.eval_metric]


def _graphed_epoch(loader, model, loss_fn, prediction_fn, evaluator):
    """The GraphedEpoch of (model, loader) and these loss / metric objects, kept on the loader; None for a loader that is not padded."""
    from .loader import PaddedDataLoader
    if not isinstance(loader, PaddedDataLoader):
        return None
    held = loader.graphed_epochs
    key = (id(model), _loss_name(loss_fn), _metric_name(prediction_fn), None if evaluator is None else (id(evaluator), evaluator.name))
    ep = held.get(key)
    if ep is None or ep.model is not model or ep.evaluator is not evaluator:
        ep = held[key] = GraphedEpoch(model, loader, loss_fn, prediction_fn, evaluator)
    return ep


def test(loader, model, loss_fn, device, prediction_fn=None, n_iters=None):
    """train_test_funcs.py:177-206: ``(sum_b loss_b * num_graphs_b / len(loader.dataset), sum_b metric_b / len(loader.dataset))`` with one
    host read, at the end.  Over a ``loader.PaddedDataLoader``: the same through a :class:`GraphedEpoch` kept on the loader."""
    model.eval()
    graphed = _graphed_epoch(loader, model, loss_fn, prediction_fn, None)
    if graphed is not None:
        return graphed.run(n_iters)
    loss, metric = _loss_name(loss_fn), _metric_name(prediction_fn)
    acc = None
    with torch.no_grad():
        for data in _batches(loader, n_iters):
            data = data.to(device)
            y_hat = model(data)
            if acc is None:
                acc = EpochAccumulator(0, y_hat.shape[-1] if y_hat.dim() >= 2 else 1, 1, loss, metric, device=y_hat.device, keep_rows=False)
            acc.add(y_hat, data.y, data.num_graphs)
    n = len(loader.dataset)
    if acc is None:
        return 0 / n, 0 / n
    r = acc.result()
    return r.weighted_loss_sum / n, r.metric_sum / n


def test_ogb(loader, model, loss_fn, device, evaluator, n_iters=None):
    """train_test_funcs.py:209-259: ``(sum_b loss_b * num_graphs_b / len(loader.dataset), evaluator.eval(...)[evaluator.eval_metric])``.
    Rows are gathered on the device; a batch whose ``x`` has one row is skipped (:230); ``ogbg-ppa`` takes the arg-max of the
    predictions (:236-238) and, as the training loop does (:96), ``loss_fn(pred, y.view(-1))``.  Over a ``loader.PaddedDataLoader``: the same
    through a :class:`GraphedEpoch` kept on the loader."""
    model.eval()
    graphed = _graphed_epoch(loader, model, loss_fn, None, evaluator)
    if graphed is not None:
        return graphed.run(n_iters)
    loss = _loss_name(loss_fn)
    ppa = evaluator.name == "ogbg-ppa"
    acc = None
    with torch.no_grad():
        n_batches = len(loader) if n_iters is None else n_iters
        for batch in _batches(loader, n_iters):
            batch = batch.to(device)
            if batch.x.shape[0] == 1:
                continue
            pred = model(batch)
            if acc is None:
                rows = len(loader.dataset) * max(1, -(-n_batches // max(len(loader), 1)))       # the dataset once per pass over the loader
                acc = EpochAccumulator(rows, pred.shape[1], pred.shape[1], loss, None, device=pred.device)
            acc.add(pred, batch.y.view(-1) if ppa else batch.y.view(pred.shape), batch.num_graphs)
    if acc is None:
        raise RuntimeError("test_ogb: no batch to evaluate")
    r = acc.result()
    y_true, y_pred = r.y_true, r.y_pred
    if ppa:
        y_pred = torch.argmax(y_pred, dim=1).view(-1, 1)
    if not isinstance(evaluator, Evaluator):          # a foreign evaluator (ogb's own): numpy arrays, copied once
        y_true, y_pred = y_true.cpu().numpy(), y_pred.cpu().numpy()
    return r.weighted_loss_sum / len(loader.dataset), evaluator.eval({"y_true": y_true, "y_pred": y_pred})[evaluator.eval_metric]
