"""HIP-graph replay of a fixed-shape step (the reference's real batch sizes are 32-128 graphs).

At those sizes a step is ~10 small dependent launches and the time goes to enqueueing them from Python (bench.py `small_batch`: 120 us eager
at B = 128).  Every launch of this package goes to PyTorch's current stream, so a step can be captured once and replayed (66-72 us):

    step = gsn_amd.graphs.GraphedStep(lambda: model_forward(static_x, static_ei, ...))   # warm-up on a side stream, then capture
    static_x.copy_(new_x); ...                                                          # refill the SAME input tensors
    y = step()                                                                          # one hipGraphLaunch; y is the captured output

Rules of stream capture apply: shapes, pointers and launch arguments are frozen (re-capture for another batch shape), nothing inside the step
may synchronise (status read-backs are deferred or off: `check=False` for the CSR build, the embedding status ring).  Caches keyed on
PARAMETERS (prepared weights, constant rows) are filled by the warm-up runs and stay valid; caches keyed on the INPUT tensors (the
aggregation index of `edge_index`, readout index pairs, graph sizes) are dropped right before the capture, so that the kernels that build
them become nodes of the graph: a replay after `static_edge_index.copy_(new_batch)` rebuilds them from the new contents.
"""
from __future__ import annotations

import torch


class GraphedStep:
    """Capture ``fn()`` (no arguments: it closes over its static input tensors) into a HIP graph; calling the object replays it and
    returns the outputs of the captured run (the same tensor objects every time -- copy them out before the next replay if needed)."""

    def __init__(self, fn, warmup: int = 3, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        from . import flags, layers
        layers.drop_input_caches()                     # (the index builds of the static inputs are recorded, not looked up)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.outputs = fn()
        layers.drop_input_caches()                     # (what the capture cached lives in graph-pool memory no eager call has written:
        layers.drop_capture_caches()                   #  indices of the inputs, and the derived weights keyed on the parameters' versions)
        self.replays = 0

    def __call__(self):
        self.graph.replay()
        self.replays += 1
        return self.outputs

    replay = __call__


class GraphedTrainStep:
    """One whole training step -- ``optimizer.zero_grad(); loss = loss_fn(); loss.backward(); all-reduce; optimizer.step()``
    (train_test_funcs.py:88-106) -- captured into ONE HIP graph and replayed with one launch.

    At the reference's batch sizes (README.md:112, :121: 128 / 32 graphs) a step is several hundred launches of a few microseconds
    each; eager, its time is the Python in front of them (profiles/r03_train_step_progress.txt: 6.6 ms at B = 32 of which < 1 ms is
    device time).  Captured, forward, the native adjoints, the gradient bucket (+ the RCCL all-reduce when the process group has more
    than one rank) and the optimizer's multi-tensor update are nodes of one graph.

        step = GraphedTrainStep(lambda: loss_fn(model(data), data.y), optimizer)     # `data`: static tensors, refilled with copy_()
        loss = step()                                                                # replay; `loss` is the captured 0-d tensor

    What stays correct across replays, and why:
      * BatchNorm running statistics and ``num_batches_tracked`` live on the device and are advanced by the captured kernels;
      * dropout draws from PyTorch's generator, whose Philox offset the graph advances per replay (a replay is not a repeat); native
        dropout (gsn_amd.dropout) reads its call counter from device memory, so a replay draws the masks an eager step at the same state
        would draw;
      * the parameters are updated in place by the captured optimizer kernels, which PyTorch's version counters do not see: the
        derived-weight caches of gsn_amd.layers are keyed on those counters, so every replay bumps them -- parameters and the BatchNorm
        buffers the captured kernels write (torch.autograd.graph.increment_version -- no launch) -- and an eager forward after a replay
        prepares its weights and eval-mode BatchNorm vectors afresh;
      * the learning rate, with gsn_amd.optim.Adam: its kernel reads it from device memory, uploaded here when a scheduler changed it.
    The warm-up steps are REAL steps (they update the parameters); shapes are frozen: capture one object per batch shape.
    Optimizers with a host-side step counter (Adam, AdamW ...) must be built with ``capturable=True``."""

    def __init__(self, loss_fn, optimizer, parameters=None, warmup: int = 3, allreduce: bool = True, average: bool = True, group=None,
                 force_allreduce: bool = False, device=None):
        from . import dist as gdist
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if optimizer.defaults.get("capturable") is False:
            raise ValueError("GraphedTrainStep: build %s with capturable=True (its step counter must live on the device)" % type(optimizer).__name__)
        self.optimizer = optimizer
        self.params = [p for g in optimizer.param_groups for p in g["params"]] if parameters is None else list(parameters)

        def step():
            optimizer.zero_grad(set_to_none=True)
            loss = loss_fn()
            loss.backward()
            if allreduce:
                gdist.allreduce_gradients(self.params, average=average, group=group, force=force_allreduce)
            optimizer.step()
            return loss.detach()

        self._eager = step
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)          # (the captured backward allocates the gradients from the graph's pool)
        from . import flags, layers
        flags.RAW_WRITTEN = []
        # caches keyed on the INPUT tensors (aggregation index, readout pairs, graph sizes) were filled by the warm-up steps: dropped, so
        # that their builds are recorded -- a replay after data.edge_index.copy_(new_batch) then runs them on the new contents
        layers.drop_input_caches()
        try:
            with torch.cuda.graph(self.graph):
                self.loss = step()
            seen, extra = set(id(p) for p in self.params), []
            for t in flags.RAW_WRITTEN:               # BatchNorm running statistics / counters the captured kernels update in place
                if id(t) not in seen:
                    seen.add(id(t))
                    extra.append(t)
            self._bump = self.params + extra
        finally:
            flags.RAW_WRITTEN = None
        # what the capture cached -- derived weights keyed on the parameters' versions, indices of the inputs -- lives in graph-pool memory
        # that nothing has written yet (a capture records): an eager forward before the first replay must not find it
        layers.drop_input_caches()
        layers.drop_capture_caches()
        torch.autograd.graph.increment_version(self._bump)
        self.replays = 0
        self.steps_taken = max(1, warmup)              # (a capture records, it does not execute)

    def __call__(self):
        sync = getattr(self.optimizer, "sync_hyperparameters", None)      # (gsn_amd.optim.Adam: the rate a scheduler wrote since)
        if sync is not None:
            sync()
        self.graph.replay()
        torch.autograd.graph.increment_version(self._bump)
        self.replays += 1
        self.steps_taken += 1
        return self.loss

    replay = __call__


class PaddedTrainStep:
    """Training over a ``loader.PaddedDataLoader``: one collate launch and ONE graph replay per batch.

    ``step(batch)`` takes a batch of the loader.  A padded batch runs the captured step -- forward under ``loader.masked_training(batch)``
    (BatchNorm statistics over the real rows, counted on the device), the masked loss with ``n_valid`` (pad graphs contribute nothing and
    get zero gradient rows), backward, the gradient all-reduce and the optimizer -- captured ONCE, on the first padded batch, through
    :class:`GraphedTrainStep` over the loader's static tensors (``captures``); every padded batch, the first included, is a replay
    (``replays``).  A batch that did not fit the loader's capacities comes as an ordinary ``Batch`` and takes the same step eagerly
    (``eager_batches``).  ``run_epoch()`` iterates the loader and returns the batch losses (a 1-D device tensor, no host read).

    ``loss``: a kind of ``evaluation.masked_loss`` ("BCEWithLogitsLoss", "L1Loss", "MSELoss", "CrossEntropyLoss"), an
    ``evaluation.MaskedLoss``, or a callable ``loss(y_hat, y, n_valid=None)``.  ``optimizer``: ``gsn_amd.optim.Adam`` or a capturable
    optimizer, as for GraphedTrainStep.

    The warm-up steps GraphedTrainStep takes before it captures are real steps; here they do not count: parameters, buffers and the
    optimizer's state tensors are put back afterwards (an optimizer state that did not exist before is zeroed in place, the fresh state of
    the Adam family), so the first replay is the first step.  What is NOT put back is random-number state: with dropout the warm-up has
    drawn masks.

    Refusals are decided from the host numbers of the batch before the replay: exactly one real row in a row class that feeds a
    train-mode BatchNorm raises the ``ValueError`` torch raises.  The model must be in training mode."""

    def __init__(self, model, loader, loss, optimizer, parameters=None, warmup: int = 1, allreduce: bool = True, average: bool = True,
                 group=None, force_allreduce: bool = False):
        from .loader import PaddedDataLoader
        if not isinstance(loader, PaddedDataLoader):
            raise TypeError("PaddedTrainStep: a loader.PaddedDataLoader (batches of fixed shape in static tensors), not %s" % type(loader).__name__)
        from . import evaluation
        if isinstance(loss, str):
            evaluation._kind_of(loss)
            self._loss = lambda y_hat, y, n_valid=None, _k=loss: evaluation.masked_loss(_k, y_hat, y, n_valid=n_valid)
        elif callable(loss):
            self._loss = loss
        else:
            raise TypeError("PaddedTrainStep: loss is a loss kind, an evaluation.MaskedLoss or a callable (y_hat, y, n_valid=None)")
        self.model, self.loader, self.optimizer = model, loader, optimizer
        self.params = [p for g in optimizer.param_groups for p in g["params"]] if parameters is None else list(parameters)
        self._graph_kw = dict(warmup=max(1, int(warmup)), allreduce=allreduce, average=average, group=group, force_allreduce=force_allreduce)
        self.graphed = None
        self._bn_rows = {}                # row class -> width of a train-mode BatchNorm it feeds (noted by the captured forward)
        self.captures = self.replays = self.eager_batches = 0

    # ---- the step, eager -------------------------------------------------------------------------------------------------------------
    def _forward_loss(self, batch):
        from .loader import masked_training
        if getattr(batch, "padded", False):
            with masked_training(batch) as bounds:
                pred = self.model(batch)
            for cls, b in bounds.items():
                if b.used:
                    self._bn_rows[cls] = int(b.used)
            return self._loss(pred, batch.y, n_valid=batch.n_valid)
        return self._loss(self.model(batch), batch.y)

    def _eager(self, batch):
        from . import dist as gdist
        kw = self._graph_kw
        self.optimizer.zero_grad(set_to_none=True)
        loss = self._forward_loss(batch)
        loss.backward()
        if kw["allreduce"]:
            gdist.allreduce_gradients(self.params, average=kw["average"], group=kw["group"], force=kw["force_allreduce"])
        self.optimizer.step()
        return loss.detach()

    # ---- capture -----------------------------------------------------------------------------------------------------------------------
    def _capture(self, batch):
        model, opt = self.model, self.optimizer
        keep = [(t, t.detach().clone()) for t in list(model.parameters()) + list(model.buffers())]
        known = {id(t) for t, _ in keep}
        keep += [(p, p.detach().clone()) for p in self.params if id(p) not in known]
        keep_state = {(id(p), k): v.detach().clone() for p, st in opt.state.items() for k, v in st.items() if isinstance(v, torch.Tensor)}
        try:
            self.graphed = GraphedTrainStep(lambda: self._forward_loss(batch), opt, self.params, device=batch.n_valid.device, **self._graph_kw)
        finally:
            # put back whatever the warm-up steps moved -- also when one of them raised (a refusal inside the first forward): the steps
            # before it must not stay applied
            with torch.no_grad():
                for t, v in keep:
                    t.copy_(v)
                for p, st in opt.state.items():
                    for k, v in st.items():
                        if isinstance(v, torch.Tensor):
                            old = keep_state.get((id(p), k))
                            v.copy_(old) if old is not None else v.zero_()
        self.captures += 1

    def _refuse(self, batch):
        rows = {"graph": batch.num_real_graphs, "vertex": batch.num_real_nodes, "edge": batch.num_real_edges}
        for cls, width in self._bn_rows.items():
            if int(rows[cls]) == 1:
                raise ValueError("Expected more than 1 value per channel when training, got input size torch.Size([1, %d])" % width)

    # ---- the public loop ---------------------------------------------------------------------------------------------------------------
    def step(self, batch):
        if not self.model.training:
            raise RuntimeError("PaddedTrainStep: the model is in evaluation mode (call model.train(); evaluation.GraphedEpoch is the replayed "
                               "evaluation epoch)")
        if not getattr(batch, "padded", False):
            loss = self._eager(batch)
            self.eager_batches += 1
            return loss
        if batch is not self.loader._batch:
            raise ValueError("PaddedTrainStep: the padded batch of another loader (the captured step reads this loader's static tensors)")
        self._refuse(batch)
        if self.graphed is None:
            self._capture(batch)
        loss = self.graphed()
        self.replays += 1
        return loss

    __call__ = step

    def run_epoch(self):
        """One pass over the loader; the losses of its batches in order (1-D fp32 device tensor; empty for an empty loader)."""
        losses = [self.step(batch).clone() for batch in self.loader]
        dev = self.loader._batch.n_valid.device
        return torch.stack(losses) if losses else torch.empty(0, dtype=torch.float32, device=dev)
