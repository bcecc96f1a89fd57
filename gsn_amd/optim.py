"""Native Adam: ``torch.optim.Adam`` (train_test_funcs.py:22, :106) as ONE HIP launch per ``step()`` (csrc/optim.hip).

    opt = gsn_amd.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    sched = torch.optim.lr_scheduler.StepLR(opt, 50, gamma=0.5)          # torch's schedulers: they only read and write param_groups

The kernel reads the learning rate (and betas, eps, weight decay) from a float64 device record per parameter group and the step counters
from a device array, so a step captured into a HIP graph (``gsn_amd.graphs.GraphedTrainStep``) follows ``StepLR`` / ``ReduceLROnPlateau``:
``sync_hyperparameters()`` -- called by ``GraphedTrainStep`` in front of every replay, and by every eager ``step()`` -- uploads a group's
record when ``param_groups[i]`` differs from what the device holds.  ``torch.optim.Adam(capturable=True)`` bakes the rate into the capture.

State is interchangeable with ``torch.optim.Adam`` at the ``state_dict`` level, in both directions.  It lives in two flat fp32 buffers
(``exp_avg``, ``exp_avg_sq``) and one fp32 ``[P]`` array of step counters; ``self.state[p]`` holds views into them.  There is no CPU
fallback: construction and state dicts work on any device, ``step()`` needs the parameters on a GPU."""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _abi

CHUNK_ELEMS = 8192          # GSN_ADAM_CHUNK_ELEMS (include/gsn_abi.h): elements one workgroup updates
_TENSOR_WORDS = 6           # GSN_ADAM_TENSOR_WORDS: parameter, gradient, exp_avg offset, exp_avg_sq offset, elements, group
_GROUP_DOUBLES = 8          # GSN_ADAM_GROUP_DOUBLES: lr, beta1, beta2, eps, weight_decay, decoupled, 0, 0
_MAX_ELEMS = 2 ** 31 - 1
_NO_FALLBACK = ("gsn_amd.optim.Adam.step: the parameters are on %s; the update is a HIP kernel (gfx950) and there is no CPU fallback")


def chunk_table(sizes, chunk: int = CHUNK_ELEMS) -> np.ndarray:
    """int32 ``[n_chunks, 2]``: (tensor, first element) of every workgroup of the launch.  Tensor ``i`` of ``sizes[i]`` elements gets
    ``ceil(sizes[i] / chunk)`` chunks in order: every element lies in exactly one chunk, no chunk crosses a tensor, an empty tensor has none."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if sizes.size and (sizes.min() < 0 or sizes.max() > _MAX_ELEMS):
        raise ValueError("chunk_table: sizes must lie in [0, 2^31 - 1]")
    counts = (sizes + (chunk - 1)) // chunk
    tensor = np.repeat(np.arange(sizes.size, dtype=np.int64), counts)
    first = (np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)) * chunk
    return np.stack([tensor, first], axis=1).astype(np.int32).reshape(-1, 2)


class _Staging:
    """Uploads of one small host table: each comes from a pinned slot that no copy in flight can still be reading (a ring; a slot is
    rewritten only behind the event of its last copy).  Inside a stream capture the copy becomes a node of the graph that re-reads its
    pinned source at every replay: it comes from a slot set aside by an earlier eager call (no pinned allocation while capturing), which
    is kept for good and never rewritten."""
    SLOTS = 4

    def __init__(self):
        self.ring, self.next, self.spare, self.kept = [], 0, None, []

    def _pinned(self, nbytes):
        return torch.empty(max(nbytes, 8), dtype=torch.uint8).pin_memory()

    def reserve(self, nbytes):
        if self.spare is None or self.spare.numel() < nbytes:
            self.spare = self._pinned(nbytes)

    def upload(self, dst, src: np.ndarray, capturing: bool):
        raw = torch.from_numpy(src.reshape(-1).view(np.uint8))
        n = raw.numel()
        if capturing:
            if self.spare is None or self.spare.numel() < n:
                raise RuntimeError("gsn_amd.optim.Adam: step() inside a stream capture needs a pinned staging slot set aside by an earlier "
                                   "eager step (run the step eagerly once before capturing it)")
            host, self.spare = self.spare, None
            self.kept.append(host)
        else:
            if len(self.ring) < self.SLOTS:
                self.ring.append([self._pinned(n), None])
            slot = self.ring[self.next % len(self.ring)]
            self.next += 1
            if slot[1] is not None:
                slot[1].synchronize()
            if slot[0].numel() < n:
                slot[0] = self._pinned(n)
            host = slot[0]
        host[:n].copy_(raw)
        dst.view(torch.uint8).reshape(-1)[:n].copy_(host[:n], non_blocking=True)
        if not capturing:
            if slot[1] is None:
                slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(dst.device))
            self.reserve(n)


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` / ``AdamW`` arithmetic (``amsgrad=False``, ``maximize=False``) in one HIP launch per step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *, amsgrad=False,
                 maximize=False, differentiable=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= float(lr):
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        # every key torch.optim.Adam.defaults has, so that state dicts interchange
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=True, differentiable=differentiable, fused=None, decoupled_weight_decay=decoupled_weight_decay)
        self._ready = False
        super().__init__(params, defaults)
        self._tables, self._hyper = _Staging(), _Staging()
        self._views, self._index = [], {}
        self._layout()
        self._ready = True

    # ---- parameter groups and state layout -------------------------------------------------------------------------------------------
    @staticmethod
    def _check_group(group, gi):
        for key in ("amsgrad", "maximize", "differentiable"):
            if group.get(key, False):
                raise ValueError("gsn_amd.optim.Adam: %s=True is not supported (the reference uses torch.optim.Adam's defaults)" % key)
        names = group.get("param_names")
        for j, p in enumerate(group["params"]):
            what = "parameter %s(index %d of group %d, shape %s)" % (("%r " % names[j]) if names else "", j, gi, tuple(p.shape))
            if p.dtype != torch.float32:
                raise TypeError("gsn_amd.optim.Adam: %s is %s; parameters must be fp32" % (what, p.dtype))
            if p.layout != torch.strided or not p.is_contiguous():
                raise TypeError("gsn_amd.optim.Adam: %s is not contiguous" % what)
            if p.numel() > _MAX_ELEMS:
                raise TypeError("gsn_amd.optim.Adam: %s has more than 2^31 - 1 elements" % what)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        try:
            self._check_group(self.param_groups[-1], len(self.param_groups) - 1)
            if getattr(self, "_ready", False):
                self._layout()
        except Exception:
            self.param_groups.pop()
            raise

    def _layout(self):
        """(Re)build the flat state buffers and the tables for the current parameter groups; state that exists is carried over."""
        params, group_of = [], []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                params.append(p)
                group_of.append(gi)
        devices = {p.device for p in params}
        if len(devices) > 1:
            raise TypeError("gsn_amd.optim.Adam: parameters must be on one device, got %s" % sorted(str(d) for d in devices))
        dev = devices.pop() if devices else torch.device("cpu")
        sizes = np.array([p.numel() for p in params], dtype=np.int64)
        padded = (sizes + 3) & ~3                      # (every state slot starts on a 16-byte boundary of its flat buffer)
        offs = np.cumsum(padded) - padded
        total = int(padded.sum())
        exp_avg = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        exp_avg_sq = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        steps = torch.zeros(max(len(params), 1), dtype=torch.float32, device=dev)
        views, index = [], {}
        for i, p in enumerate(params):
            o, n = int(offs[i]), int(sizes[i])
            v = {"step": steps[i], "exp_avg": exp_avg[o:o + n].view(p.shape), "exp_avg_sq": exp_avg_sq[o:o + n].view(p.shape)}
            j = self._index.get(id(p))
            if j is not None:
                for k in v:
                    v[k].copy_(self._views[j][k])
            views.append(v)
            index[id(p)] = i
        for p in list(self.state.keys()):
            self.state[p] = views[index[id(p)]]
        self._params, self._group_of, self._device = params, group_of, dev
        self._exp_avg, self._exp_avg_sq, self._steps = exp_avg, exp_avg_sq, steps
        self._views, self._index = views, index
        self._max_elems = int(sizes.max()) if len(params) else 0
        chunks = chunk_table(sizes)
        self._n_chunks = int(chunks.shape[0])
        P = len(params)
        self._host = np.zeros(P * _TENSOR_WORDS + self._n_chunks + 1, dtype=np.int64)      # [tensor records | chunk pairs (int32)]
        self._rec = self._host[:P * _TENSOR_WORDS].reshape(P, _TENSOR_WORDS)
        self._host[P * _TENSOR_WORDS:].view(np.int32)[:2 * self._n_chunks] = chunks.reshape(-1)
        self._rec[:, 2] = offs
        self._rec[:, 3] = offs
        self._rec[:, 4] = sizes
        self._rec[:, 5] = group_of
        self._uploaded = None                          # host copy of what the device table holds
        self._hyper_host = np.zeros((max(len(self.param_groups), 1), _GROUP_DOUBLES), dtype=np.float64)
        self._hyper_uploaded = None
        if dev.type == "cuda":
            self._table = torch.zeros(self._host.size, dtype=torch.int64, device=dev)
            self._groups = torch.zeros(self._hyper_host.shape, dtype=torch.float64, device=dev)
            self._done = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            self._table = self._groups = self._done = None
        if not hasattr(self, "_captured"):
            self._captured = []                        # device tables of captured steps: a graph holds their addresses

    def flat_state(self):
        """``(exp_avg, exp_avg_sq, steps)``: the two flat fp32 state buffers and the ``[P]`` step counters that ``self.state`` views."""
        return self._exp_avg, self._exp_avg_sq, self._steps

    # ---- state dicts ------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """As ``torch.optim.Adam.state_dict()``; the tensors are copies, not views of the flat buffers."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in st.items()} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a state dict of this class or of ``torch.optim.Adam`` (``capturable`` or not: steps as 0-d tensors on either device).
        The values are copied into the flat buffers; ``self.state`` keeps holding views of them."""
        for gi, g in enumerate(state_dict["param_groups"]):
            for key in ("amsgrad", "maximize", "differentiable"):
                if g.get(key, False):
                    raise ValueError("gsn_amd.optim.Adam.load_state_dict: group %d has %s=True, which is not supported" % (gi, key))
        super().load_state_dict(state_dict)
        loaded, state = self.state, collections.defaultdict(dict)
        seen = set()
        for p, st in loaded.items():
            i = self._index[id(p)]
            v = self._views[i]
            v["step"].copy_(torch.as_tensor(st["step"], dtype=torch.float32))
            v["exp_avg"].copy_(st["exp_avg"])
            v["exp_avg_sq"].copy_(st["exp_avg_sq"])
            state[p] = v
            seen.add(i)
        for i, v in enumerate(self._views):              # a parameter the loaded dict has no state for starts from zero again
            if i not in seen:
                for t in v.values():
                    t.zero_()
        self.state = state

    # ---- the step ---------------------------------------------------------------------------------------------------------------------
    def _hyper_record(self):
        h = self._hyper_host
        for gi, g in enumerate(self.param_groups):
            b1, b2 = g["betas"]
            dec = bool(g.get("decoupled_weight_decay", False))
            h[gi, :6] = (float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), 1.0 if dec else 0.0)
        return h

    def sync_hyperparameters(self):
        """Upload the record of every group whose ``param_groups[i]`` differs from what the device holds (lr, betas, eps, weight_decay,
        decoupled flag); no launch and no copy when nothing changed.  Every eager ``step()`` does this itself; a replayed HIP graph does
        not pass through ``step()``, so ``GraphedTrainStep`` calls it in front of every replay."""
        if self._groups is None:
            return False
        h = self._hyper_record()
        if self._hyper_uploaded is not None and np.array_equal(h, self._hyper_uploaded):
            return False
        if torch._C._cuda_isCurrentStreamCapturing():
            raise RuntimeError("gsn_amd.optim.Adam: the hyper-parameters changed since their last upload and a stream capture is under way; "
                               "call sync_hyperparameters() (or run one eager step) before capturing")
        with _abi.device_guard(self._device):
            self._hyper.upload(self._groups, h, False)
        self._hyper_uploaded = h.copy()
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = self._params
        dev = self._device
        if dev.type != "cuda":
            _abi.require_gpu()
            raise RuntimeError(_NO_FALLBACK % dev)
        grads, updated = [], []
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                grads.append(0)
                continue
            if g.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
            if g.dtype != torch.float32 or g.shape != p.shape or g.device != p.device or not g.is_contiguous():
                raise TypeError("gsn_amd.optim.Adam.step: the gradient of parameter %d (shape %s) must be contiguous fp32 of the parameter's "
                                "shape and device, got %s %s on %s" % (i, tuple(p.shape), g.dtype, tuple(g.shape), g.device))
            grads.append(g.data_ptr() or 16)           # (an empty tensor has no address; it has no chunk either: never dereferenced)
            updated.append(p)
        if not updated:
            return loss                                # no gradient anywhere: no launch
        for p in updated:                              # torch's lazy initialisation: state appears with the first gradient
            if p not in self.state:
                self.state[p] = self._views[self._index[id(p)]]
        rec = self._rec
        rec[:, 0] = [p.data_ptr() for p in params]
        rec[:, 1] = grads
        capturing = torch._C._cuda_isCurrentStreamCapturing()
        with _abi.device_guard(dev):
            self.sync_hyperparameters()
            if capturing:
                # the copy is recorded as a node of the graph; table and pinned source are the capture's own, so that eager steps between
                # replays (other gradient addresses) and the replays do not rewrite each other's table
                table = torch.empty_like(self._table)
                self._tables.upload(table, self._host, True)
                self._captured.append(table)
            else:
                table = self._table
                if self._uploaded is None or not np.array_equal(self._host, self._uploaded):
                    self._tables.upload(table, self._host, False)
                    self._uploaded = self._host.copy()
                else:
                    self._tables.reserve(self._host.nbytes)
            P = len(params)
            base = table.data_ptr()
            _abi.check(_abi.lib().gsn_adam_step_hip(P, base, self._n_chunks, base + 8 * P * _TENSOR_WORDS, len(self.param_groups),
                                                    self._groups.data_ptr(), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
                                                    self._steps.data_ptr(), self._done.data_ptr(), self._max_elems, _abi.current_stream()),
                       "gsn_adam_step_hip")
        # the kernel wrote through raw pointers: the derived-weight caches of gsn_amd.layers are keyed on the version counters
        torch.autograd.graph.increment_version(updated)
        return loss


def setup_optimization(model, **args):
    """train_test_funcs.py:18-35 with the native Adam: ``(optimizer, scheduler)`` for ``args['lr']``, ``args['regularization']`` and
    ``args['scheduler']`` in ``ReduceLROnPlateau`` (``decay_rate``, ``patience``), ``StepLR`` (``decay_steps``, ``decay_rate``), ``None``.
    The schedulers are torch's own (the reference's ``verbose=True`` is gone from this torch and only printed)."""
    kind = args['scheduler']
    if kind not in ('ReduceLROnPlateau', 'StepLR', 'None'):
        raise NotImplementedError('Scheduler {} is not currently supported.'.format(kind))
    optimizer = Adam(model.parameters(), lr=args['lr'], weight_decay=args['regularization'])
    scheduler = None
    if kind == 'ReduceLROnPlateau':
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=args['decay_rate'], patience=args['patience'])
    elif kind == 'StepLR':
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, args['decay_steps'], gamma=args['decay_rate'])
    return optimizer, scheduler
