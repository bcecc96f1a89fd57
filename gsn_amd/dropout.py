"""Native dropout: the reference's ``F.dropout`` calls (models_graph_classification_ogb_original.py:243-259, models_graph_classification.py:240,
directional_gsn/nets/dgn_layer.py:81, dgn_net.py:58) as ONE HIP launch per direction, the residual add included, without a mask tensor.

* ``dropout(x, p, training=True, residual=None, state=None)`` -- ``residual + mask * x / (1 - p)`` (bit for bit that fp32 expression, product
  and sum rounded separately) as one autograd node over ``gsn_dropout_fwd_hip`` / ``gsn_dropout_bwd_hip``.  The backward rebuilds the mask from
  the 16 bytes the forward left in ``used``; the residual's gradient is the incoming gradient itself.
* ``DropoutState`` -- the random stream of csrc/dropout_core.h on the device: ``(seed, calls)``, both int64.  Call number ``calls`` of seed
  ``seed`` keeps element ``e`` iff word ``e & 3`` of ``Philox4x32-10(counter = (e >> 2, calls), key = seed)`` is ``>= round(p 2^32)``.  The
  kernel advances ``calls`` itself, so a replayed HIP graph (``gsn_amd.graphs``) draws the masks an eager call at that state would draw, and
  ``set_state`` in front of a replay and of an eager step makes them draw the same ones.
* ``Dropout(p)`` -- the module.

ONE STATE SERVES ONE STREAM AT A TIME: calls that share a state must be ordered (one stream, or one captured graph), as the steps of a
``gsn_amd.optim.Adam`` must be.  There is no fallback: without a GPU the entries raise.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _abi
from ._runtime import _timed

_MASK63 = (1 << 63) - 1
_STATES = {}


def threshold(p):
    """``min(2^32 - 1, round(p 2^32))``: an element is kept iff its 32-bit word is >= this."""
    return min((1 << 32) - 1, int(round(float(p) * 4294967296.0)))


def scale(p):
    """``float32(1 / (1 - p))``: the double division, rounded once."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def _signed64(v):
    v = int(v) & ((1 << 64) - 1)
    return v - (1 << 64) if v >> 63 else v


def _cuda_device(device, who):
    dev = torch.device(device)
    _abi.require_gpu()
    if dev.type != "cuda":
        raise RuntimeError("gsn_amd.dropout: %s must live on the GPU (there is no CPU fallback)" % who)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _refuse_capture(what):
    if torch._C._cuda_isCurrentStreamCapturing():
        raise RuntimeError("gsn_amd.dropout: %s while the current stream is capturing -- the call counter must outlive the graph's memory pool; "
                           "create the state (or run one eager warm-up step, which creates the default one) before the capture" % what)


class DropoutState:
    """``(seed, calls)`` of one dropout stream, int64[2] on ``device``, and the ``done`` word of the kernels' counter scheme.

    ``seed=None``: ``torch.initial_seed() & (2^63 - 1)`` -- ``torch.manual_seed`` governs it.  Any 64-bit seed is taken (stored two's
    complement).  The forward kernel adds 1 to ``calls``; nothing on the host counts.  One state serves one stream at a time (module
    docstring).  Creating one, seeding it or setting it while the current stream is capturing raises ``RuntimeError``."""

    def __init__(self, device, seed=None):
        dev = _cuda_device(device, "a DropoutState")
        _refuse_capture("a DropoutState is created")
        self.device = dev
        seed = (torch.initial_seed() & _MASK63) if seed is None else _signed64(seed)
        self._state = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
        self._done = torch.zeros(1, dtype=torch.int32, device=dev)

    def manual_seed(self, seed):
        """Seed ``seed``, call counter 0."""
        return self.set_state(torch.tensor([_signed64(seed), 0], dtype=torch.int64))

    def get_state(self):
        """CPU int64[2] ``(seed, calls)``: one host read (checkpoints, tests)."""
        return self._state.cpu()

    def set_state(self, state):
        """Take an int64[2] ``(seed, calls)`` as ``get_state`` returns it."""
        state = torch.as_tensor(state)
        if state.dtype != torch.int64 or tuple(state.shape) != (2,):
            raise ValueError("DropoutState.set_state: an int64 tensor of 2 elements (seed, calls), got %s %s" % (state.dtype, tuple(state.shape)))
        _refuse_capture("a DropoutState is set")
        self._state.copy_(state)
        return self


def default_state(device):
    """The state the models' native dropout draws from: one per device, created at its first use."""
    dev = _cuda_device(device, "the default DropoutState")
    st = _STATES.get(dev.index)
    if st is None:
        st = _STATES[dev.index] = DropoutState(dev)
    return st


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, p, state):
        x = x.contiguous()
        res = None if residual is None else residual.contiguous()
        n = x.numel()
        ctx.consts = (n, threshold(p), scale(p) if p < 1.0 else 0.0, p >= 1.0)
        ctx.set_materialize_grads(False)          # (no zero fill for the gradient of `used`)
        if p >= 1.0:                              # everything dropped: decided here, no launch, the state stays
            out = torch.zeros_like(x) if res is None else res.clone()
            used = state._state.new_empty(0)
            ctx.mark_non_differentiable(used)
            return out, used
        out = torch.empty_like(x)
        used = torch.empty(2, dtype=torch.int64, device=x.device)
        if n:
            with _abi.device_guard(x.device), _timed("dropout_fwd", n):
                _abi.check(_abi.lib().gsn_dropout_fwd_hip(n, x.data_ptr(), _abi.ptr(res), out.data_ptr(), ctx.consts[1], ctx.consts[2],
                                                          state._state.data_ptr(), state._done.data_ptr(), used.data_ptr(), _abi.current_stream()),
                           "gsn_dropout_fwd_hip")
        ctx.save_for_backward(used)
        ctx.mark_non_differentiable(used)
        return out, used

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_used):
        if grad_out is None:
            return None, None, None, None
        n, thr, scl, all_dropped = ctx.consts
        grad_x = None
        if ctx.needs_input_grad[0]:
            if all_dropped:
                grad_x = torch.zeros_like(grad_out)
            else:
                g = grad_out.contiguous()
                grad_x = torch.empty_like(g)
                if n:
                    used, = ctx.saved_tensors
                    with _abi.device_guard(g.device), _timed("dropout_bwd", n):
                        _abi.check(_abi.lib().gsn_dropout_bwd_hip(n, g.data_ptr(), grad_x.data_ptr(), thr, scl, used.data_ptr(), _abi.current_stream()),
                                   "gsn_dropout_bwd_hip")
        return grad_x, (grad_out if ctx.needs_input_grad[1] else None), None, None


def dropout(x, p, training=True, residual=None, state=None):
    """``residual + mask * x / (1 - p)`` in training (``mask * x / (1 - p)`` without a residual), ``x + residual`` (``x``) otherwise.

    ``x``, ``residual``: fp32 GPU tensors of one shape (made contiguous when they are not).  ``state``: a ``DropoutState`` on ``x``'s device,
    default ``default_state(x.device)``.  Decided on the host: ``p`` outside [0, 1] -> ValueError; another dtype -> TypeError; a CPU tensor
    -> RuntimeError (no fallback); not training or ``p == 0`` -> no launch, the state does not advance; ``p == 1`` -> zeros (``residual``)
    with a zero gradient for ``x``, no launch, the state does not advance; an empty tensor -> no launch, the state does not advance.
    No host synchronisation, no allocation besides the output and the 16 bytes of ``used``."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
    for name, t in (("x", x), ("residual", residual)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("gsn_amd.dropout: %s must be float32, not %s" % (name, t.dtype))
    if residual is not None and residual.shape != x.shape:
        raise ValueError("gsn_amd.dropout: residual of shape %s for x of shape %s" % (tuple(residual.shape), tuple(x.shape)))
    if not x.is_cuda or (residual is not None and residual.device != x.device):
        _abi.require_gpu()
        raise RuntimeError("gsn_amd.dropout: x and residual must live on one GPU (there is no CPU fallback)")
    if not training or p == 0.0:
        return x if residual is None else x + residual
    if state is None:
        state = default_state(x.device)
    elif state.device != x.device:
        raise ValueError("gsn_amd.dropout: the DropoutState lives on %s, x on %s" % (state.device, x.device))
    return _DropoutFn.apply(x, residual, p, state)[0]


class Dropout(nn.Module):
    """``nn.Dropout(p)`` over ``dropout``: ``forward(x, residual=None)``; ``state=None`` draws from the device's default state."""

    def __init__(self, p=0.5, state=None):
        super().__init__()
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
        self.p = float(p)
        self.state = state

    def forward(self, x, residual=None):
        return dropout(x, self.p, self.training, residual, self.state)

    def extra_repr(self):
        return "p=%g" % self.p


def resolve_impl(impl):
    """``dropout_impl`` of a model: "torch" or "native"; None -> what ``flags.DROPOUT_NATIVE`` (GSN_DROPOUT) says."""
    from . import flags
    if impl is None:
        return "native" if flags.DROPOUT_NATIVE else "torch"
    if impl not in ("torch", "native"):
        raise ValueError("dropout_impl %r (one of 'torch', 'native')" % (impl,))
    return impl
