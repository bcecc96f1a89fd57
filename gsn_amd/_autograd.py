"""Native adjoints of the dense stages composed under autograd (gsn_bn_act_bwd_hip, gsn_wgrad_hip, the forward kernels on W^T), the folded
first weight of update_fn, gathered edge rows, code-gather stages, and the two generic HIP-forward autograd functions."""
from __future__ import annotations

import torch

from . import _abi, _bound, flags
from ._caches import _note_cache
from ._dense import _Stage, _block_array, _bn_batch_vectors, _bn_eval_vectors, _bn_resolve, _f16x3_takes, _linear_hip
from ._index import _csr_for, propagate
from ._runtime import _ACT_CODE, _f32c, _timed, _zeros

# native backward of dense stage lists (inputs = plain row-major blocks): gsn_bn_act_bwd_hip, gsn_wgrad_hip and the forward linear kernel
# on W^T for the input gradient
PLAIN, AFFINE, BN_BATCH, BN_RUNNING = range(4)
_BN_ROWS = (BN_BATCH, BN_RUNNING)


class _StageRec:
    """One ``Linear (+BatchNorm) (+activation)`` stage of a _DenseStagesFn call, built once per call by ``_layout``.

    ``kind``: PLAIN; AFFINE (BatchNorm on its running statistics, gamma / beta frozen: a per-column affine map in the epilogue of the product);
    BN_BATCH (batch statistics: train mode, or no running statistics); BN_RUNNING (running statistics with gradients for gamma / beta).  The
    last two materialise their pre-BN rows.  ``w_i, b_i, g_i, beta_i``: the positions of weight, bias, gamma and beta in ``tensors`` (blocks of
    stage 0, then per stage weight, [bias], [gamma, beta]; None: the stage has none).  ``act``: the activation's code.

    What forward kept for the adjoint, as indices into ``ctx.saved_tensors`` (None: not kept): ``h`` the pre-BN rows, ``y`` the fp32 output
    (None on a BatchNorm stage: the output was written as fp16 planes only), ``mean, invstd, scale, shift`` the BatchNorm vectors (AFFINE:
    ``scale`` alone).  ``x_scratch``: the forward product's row scratch (the fp16 planes of the stage's input rows, kept when the weight
    wants a gradient and the product ran on the fp16x3 kernel: gsn_wgrad_f16x3_hip multiplies it with the planes of gH) -- held here and NOT
    given to save_for_backward: saved-tensor hooks never saw it."""
    __slots__ = ("kind", "bn", "act", "n_out", "k_total", "w_i", "b_i", "g_i", "beta_i", "h", "y", "mean", "invstd", "scale", "shift", "x_scratch")

    def __init__(self, st, tensors):
        put = lambda t: tensors.append(t) or len(tensors) - 1
        bn = st.bn
        self.bn, self.act = bn, _ACT_CODE[st.act]
        self.n_out, self.k_total = st.weight.shape
        if bn is None or bn.training or bn.running_mean is None:
            self.kind = PLAIN if bn is None else BN_BATCH
        else:
            self.kind = BN_RUNNING if bn.affine and (bn.weight.requires_grad or bn.bias.requires_grad) else AFFINE
        self.w_i = put(st.weight)
        self.b_i = None if st.bias is None else put(st.bias)
        self.g_i, self.beta_i = (put(bn.weight), put(bn.bias)) if bn is not None and bn.affine else (None, None)
        self.h = self.y = self.mean = self.invstd = self.scale = self.shift = self.x_scratch = None


def _layout(stages):
    """``(records, tensors)`` of a stage list, the one walk of the tensor positions: the ``records[0].w_i`` blocks of stage 0, then what each record puts."""
    tensors = [d for d, _ in stages[0].blocks]
    return [_StageRec(st, tensors) for st in stages], tensors


# --- route decisions: each stated once -------------------------------------------------------------------------------
def _plane_rows(n_out, ptr):
    """Can a BatchNorm pass write rows of this width at this address as fp16 planes (a row scratch of the fp16x3 kernel) instead of fp32 rows?"""
    return n_out % 4 == 0 and n_out <= 640 and ptr % 16 == 0


def _output_as_planes(rec, nxt, want_w_next, m_rows, h):
    """The stage output only feeds the next product (on the fp16x3 kernel) and, in the backward pass, that product's plane weight gradient:
    BatchNorm + activation write the row scratch of Y -- no fp32 Y, no pre-pass over it (gsn_bn_act_planes_hip)."""
    return (flags.BN_ACT_PLANES and nxt is not None and _plane_rows(rec.n_out, h.data_ptr()) and flags.WGRAD_F16X3 and want_w_next
            and _f16x3_takes(m_rows, nxt.n_out, [rec.n_out], stats=nxt.kind == BN_BATCH))


def _gh_as_planes(rec, bound, want_w, need_x, m_rows, g, h):
    """A BatchNorm stage whose gH is read as fp16 planes only -- by the input-gradient product on the fp16x3 kernel (or by nobody) and by the
    plane weight gradient: the adjoint pass writes gH's row scratch and no fp32 gH (gsn_bn_act_bwd_planes_hip).  Not under a bound: there fp32
    gH with +0 pad rows, split by gsn_linear_f16x3_split_rows_hip where wanted."""
    return (bound is None and flags.BN_BWD_PLANES and rec.kind in _BN_ROWS and want_w and rec.x_scratch is not None and _plane_rows(rec.n_out, g.data_ptr())
            and (not need_x or _f16x3_takes(m_rows, rec.k_total, [rec.n_out], aligned=h.data_ptr() % 16 == 0)))


def _split_gh_alone(rec, xs, g_scr, gh, m_rows):
    """No input-gradient product on the fp16x3 kernel left the planes of gH beside the weight gradient: a pre-pass of its own makes them."""
    return xs is not None and not g_scr and rec.n_out % 4 == 0 and gh is not None and gh.data_ptr() % 16 == 0 and m_rows >= flags.WGRAD_F16X3_SPLIT_ROWS


def _fused_finalize_act(bound, m_rows):
    """Finalize + normalise + activate in one launch, where a launch costs more than the pass (never under a bound: the bounded finalize has no such form)."""
    return bound is None and 1 < m_rows <= flags.FUSE_BN_ACT_ROWS


def _weight_transposed(w, m_rows):
    """W as the input-gradient product gX = gH W reads it.  The fp16x3 kernel prepares its planes from any strides; the bf16x6 kernel stages a
    strided W with scalar loads -- fine where a launch costs more than the staging (small batches), a copy + float4 staging above."""
    if w.shape[1] > flags.LINEAR_F16X3_MIN_N or m_rows <= 16384:
        return w.detach().t()
    return w.detach().to(torch.float32).t().contiguous()


# --- the steps of a stage --------------------------------------------------------------------------------------------
def _bn_vectors(rec, h, stats, m_rows, bound):
    """Statistics -> vectors of a BatchNorm stage: ``([mean, scale, shift], invstd, y)``, ``y`` the stage output where the finalize launch wrote it too."""
    y = None
    if rec.kind == BN_BATCH:
        fused = _fused_finalize_act(bound, m_rows)
        y = torch.empty_like(h) if fused else None
        params, invstd = _bn_batch_vectors(rec.bn, h.device, lambda: stats, m_rows, True, fuse_act=(h, rec.act, y) if fused else None, bound=bound,
                                           h=h if bound is not None else None)
    else:
        params, invstd = _bn_eval_vectors(rec.bn)
    return [_f32c(v) for v in params], invstd.contiguous(), y


def _normalise(rec, as_planes, h, vecs, m_rows):
    """act(bn(h)) as a launch of its own: ``(y, None)``, or ``(None, row scratch of y)`` when the output goes to planes only."""
    L = _abi.lib()
    head = (m_rows, rec.n_out, h.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), vecs[2].data_ptr(), rec.act)
    with _abi.device_guard(h.device), _timed("bn_act", 8.0 * h.numel()):
        if as_planes:
            planes = torch.empty(int(L.gsn_linear_f16x3_scratch_bytes(m_rows, rec.n_out)), dtype=torch.uint8, device=h.device)
            _abi.check(L.gsn_bn_act_planes_hip(*head, None, planes.data_ptr(), _abi.current_stream()), "gsn_bn_act_planes_hip")
            return None, planes
        y = torch.empty_like(h)
        _abi.check(L.gsn_bn_act_hip(*head, y.data_ptr(), _abi.current_stream()), "gsn_bn_act_hip")
        return y, None


def _bn_act_adjoint(rec, kept, g, gbias, sums, bound, m_rows, as_planes):
    """gY -> gH through the activation and the BatchNorm of a stage; the column sums for gamma / beta go to ``sums``, the bias gradient to
    ``gbias``.  Returns ``(gH, None)``, or ``(None, row scratch of gH)``.  BatchNorm stages take the activation's derivative from z
    recomputed out of the pre-BN rows (the stage output is not read again); the others read the stage output."""
    L = _abi.lib()
    n_out, dev = rec.n_out, g.device
    gh = None if as_planes else torch.empty((m_rows, n_out), dtype=torch.float32, device=dev)
    gh_scratch = None
    with _abi.device_guard(dev), _timed("bn_act_bwd", 16.0 * m_rows * n_out):
        if rec.kind in _BN_ROWS:
            head = (kept[rec.h].data_ptr(), kept[rec.mean].data_ptr(), kept[rec.invstd].data_ptr(), kept[rec.scale].data_ptr(),
                    kept[rec.shift].data_ptr(), 1 if rec.kind == BN_BATCH else 2, rec.act, sums.data_ptr())
            if as_planes:
                gh_scratch = torch.empty(int(L.gsn_linear_f16x3_scratch_bytes(m_rows, n_out)), dtype=torch.uint8, device=dev)
                name, tail = "gsn_bn_act_bwd_planes_hip", (gh_scratch.data_ptr(), gbias.data_ptr())
            elif bound is not None:
                name, tail = "gsn_bn_act_bwd_from_h_bounded_hip", (gh.data_ptr(), gbias.data_ptr(), *bound.pointers())
            else:
                name, tail = "gsn_bn_act_bwd_from_h_hip", (gh.data_ptr(), gbias.data_ptr())
        else:
            name, tail = "gsn_bn_act_bwd_hip", (gh.data_ptr(), gbias.data_ptr())
            head = (kept[rec.y].data_ptr(), None, None, None, None if rec.scale is None else kept[rec.scale].data_ptr(), 0, rec.act, None)
        rc = getattr(L, name)(m_rows, n_out, g.data_ptr(), *head, *tail, _abi.current_stream())
    _abi.check(rc, name)
    return gh, gh_scratch


def _input_rows(prev, kept, blocks0, m_rows):
    """The fp32 input rows of the stage behind ``prev`` (None: stage 0's blocks); where ``prev`` wrote planes only, made again from its pre-BN rows."""
    if prev is None:
        return blocks0
    if prev.y is not None:
        return [kept[prev.y]]
    h = kept[prev.h]
    y = torch.empty_like(h)
    with _abi.device_guard(h.device):
        _abi.check(_abi.lib().gsn_bn_act_hip(m_rows, h.shape[1], h.data_ptr(), kept[prev.mean].data_ptr(), kept[prev.scale].data_ptr(),
                                             kept[prev.shift].data_ptr(), prev.act, y.data_ptr(), _abi.current_stream()), "gsn_bn_act_hip")
    return [y]


def _weight_gradient(rec, gw, gh, xs, g_scr, xin_rows, gather, m_rows):
    """gW = gH^T X into the zero-filled ``gw``: the plane kernel on the two row scratches (``g_scr``: gH's, if a product or the adjoint left
    it; ``xs``: the forward product's), else gsn_wgrad_hip on fp32 rows -- ``xin_rows()`` makes them, gathered blocks read where they lie."""
    L = _abi.lib()
    dev, n_out, k_total = gw.device, rec.n_out, rec.k_total
    if _split_gh_alone(rec, xs, g_scr, gh, m_rows):
        sc = torch.empty(int(L.gsn_linear_f16x3_scratch_bytes(m_rows, n_out)), dtype=torch.uint8, device=dev)
        one = _block_array([(gh, None)], [])
        with _abi.device_guard(dev):
            _abi.check(L.gsn_linear_f16x3_split_rows_hip(m_rows, 1, one, sc.data_ptr(), _abi.current_stream()), "gsn_linear_f16x3_split_rows_hip")
        g_scr.append(sc)
    if xs is not None and g_scr:
        with _abi.device_guard(dev), _timed("wgrad", 2.0 * m_rows * n_out * k_total):
            _abi.check(L.gsn_wgrad_f16x3_hip(m_rows, n_out, k_total, g_scr[0].data_ptr(), xs.data_ptr(), gw.data_ptr(), _abi.current_stream()),
                       "gsn_wgrad_f16x3_hip")
        return
    xin = xin_rows()
    keep = []
    modes = [None] * len(xin) if gather is None else gather[2]
    arr = _block_array([(t, None if m is None else gather[0][m]) for t, m in zip(xin, modes)], keep)
    with _abi.device_guard(dev), _timed("wgrad", 2.0 * m_rows * n_out * k_total):
        _abi.check(L.gsn_wgrad_hip(m_rows, n_out, gh.data_ptr(), len(xin), arr, gw.data_ptr(), _abi.current_stream()), "gsn_wgrad_hip")


def _block_gradients(grads, blocks0, wants, gather, gx):
    """gX of stage 0 handed to its blocks: column slices; for a block gathered through edge_index[mode] the per-edge gradients summed per vertex."""
    o = 0
    for bi, t in enumerate(blocks0):
        wd = t.shape[1]
        if wants[bi]:
            mode = None if gather is None else gather[2][bi]
            grads[bi] = gx[:, o:o + wd] if mode is None else _segment_sum_cols(gather[0], mode, gather[1], gx, o, wd)
        o += wd


class _DenseStagesFn(torch.autograd.Function):
    """Forward: stage by stage on the linear kernel, keeping what the adjoint needs (stage outputs; pre-BN rows and batch
    statistics of train-mode BatchNorm stages).  Backward: per stage  gY -> gH (BN + activation adjoint) -> gW, gb, gX."""

    @staticmethod
    def forward(ctx, recs, gather, bound, *tensors):
        # recs, tensors: _layout of the stage list.  gather = (edge_index, n_nodes, modes) or None: the stage-0 blocks (the x_i / x_j /
        # per-end-point blocks of an edge stage) are read where they lie through edge_index[mode], by the forward product AND by the weight
        # gradient -- no assembled [E, K] copy of the rows.  bound: a _bound.RowBound or None (the rows are a padded batch, BatchNorm
        # statistics over its real rows only)
        wants = ctx.needs_input_grad[3:]
        blocks0 = tensors[:recs[0].w_i]
        if gather is not None:
            idx0 = [None if m is None else gather[0][m] for m in gather[2]]
            m_rows = gather[0].shape[1]
        else:
            idx0 = [None] * len(blocks0)
            m_rows = blocks0[0].shape[0]
        kept = []
        keep = lambda t: kept.append(t) or len(kept) - 1
        y = rows = pre = None      # the output; the next stage's input rows (where planes only: a stand-in of their shape); their row scratch
        for si, rec in enumerate(recs):
            nxt = recs[si + 1] if si + 1 < len(recs) else None
            w, b = tensors[rec.w_i], None if rec.b_i is None else tensors[rec.b_i]
            scr = [] if (flags.WGRAD_F16X3 and wants[rec.w_i] and (si > 0 or gather is None)) else None
            blks = list(zip(blocks0, idx0)) if si == 0 else [(rows, None)]
            # the product: with the epilogue of a PLAIN / AFFINE stage, or plain pre-BN rows (with their column statistics on batch statistics)
            stats = _zeros(2 * rec.n_out, torch.float64, w.device).view(2, rec.n_out) if rec.kind == BN_BATCH else None
            epilogue = _bn_eval_vectors(rec.bn)[0] if rec.kind == AFFINE else (None, None, None)
            out = _linear_hip(blks, w, b, *epilogue, 0 if rec.kind in _BN_ROWS else rec.act, m_rows, out=True, stats=stats, scratch_out=scr, presplit=pre)
            if pre is not None and scr is not None and not scr:      # (rows split already by the stage before: that scratch is this product's)
                scr.append(pre)
            rec.x_scratch = scr[0] if scr else None
            pre = None
            if rec.kind in _BN_ROWS:
                vecs, invstd, y = _bn_vectors(rec, out, stats, m_rows, bound)
                if y is None:
                    y, pre = _normalise(rec, _output_as_planes(rec, nxt, nxt is not None and wants[nxt.w_i], m_rows, out), out, vecs, m_rows)
                rec.h = keep(out)
                rec.y = None if y is None else keep(y)
                rec.mean, rec.invstd, rec.scale, rec.shift = keep(vecs[0]), keep(invstd), keep(vecs[1]), keep(vecs[2])
                rows = out if y is None else y
            else:
                y = rows = out
                rec.y = keep(y)
                if rec.kind == AFFINE:
                    rec.scale = keep(_f32c(epilogue[1]))
        ctx.recs, ctx.gather, ctx.bound, ctx.m_rows, ctx.n_kept = recs, gather, bound, m_rows, len(kept)
        ctx.save_for_backward(*kept, *tensors)
        return y

    @staticmethod
    def backward(ctx, gy):
        recs, gather, m_rows = ctx.recs, ctx.gather, ctx.m_rows
        kept = ctx.saved_tensors
        tensors = kept[ctx.n_kept:]
        wants = ctx.needs_input_grad[3:]
        blocks0 = list(tensors[:recs[0].w_i])
        grads = [None] * len(tensors)
        dev = gy.device
        g = gy.to(torch.float32).contiguous()
        # every zero-initialised accumulator of this backward from two arenas (one fill each instead of three small fills per stage)
        z64 = _zeros(sum(3 * rec.n_out for rec in recs), torch.float64, dev)
        z32 = _zeros(sum(rec.n_out * rec.k_total for rec in recs if wants[rec.w_i]), torch.float32, dev)
        o64 = o32 = 0
        casts = []
        for si in range(len(recs) - 1, -1, -1):
            rec = recs[si]
            n_out = rec.n_out
            gbias, sums = z64[o64:o64 + n_out], z64[o64 + n_out:o64 + 3 * n_out].view(2, n_out)
            # (fp64 column sums -> fp32 gradients: ONE conversion of the whole arena behind the loop, the gradients are its slices)
            if rec.kind in _BN_ROWS and rec.g_i is not None:
                casts += [(rec.g_i, o64 + 2 * n_out, n_out), (rec.beta_i, o64 + n_out, n_out)]
            if rec.b_i is not None:
                casts.append((rec.b_i, o64, n_out))
            o64 += 3 * n_out
            need_x = si > 0 or any(wants[:len(blocks0)])
            want_w = wants[rec.w_i]
            bound = ctx.bound if rec.kind in _BN_ROWS else None
            h = kept[rec.h] if rec.kind in _BN_ROWS else None
            as_planes = _gh_as_planes(rec, bound, want_w, need_x, m_rows, g, h)
            gh, gh_scratch = _bn_act_adjoint(rec, kept, g, gbias, sums, bound, m_rows, as_planes)
            # input gradient first: on the fp16x3 kernel its row pre-pass leaves the fp16 planes of gH, which the weight gradient multiplies as well
            xs = rec.x_scratch if want_w else None
            g_scr = [] if xs is not None else None
            gx = None
            if need_x:
                wt = _weight_transposed(tensors[rec.w_i], m_rows)
                if as_planes:         # (the rows are split already; `h` stands in for gH's shape)
                    gx = _linear_hip([(h, None)], wt, None, None, None, None, 0, m_rows, split_k=True, presplit=gh_scratch)
                else:
                    gx = _linear_hip([(gh, None)], wt, None, None, None, None, 0, m_rows, split_k=True, scratch_out=g_scr)
            if as_planes:
                g_scr.append(gh_scratch)
            if want_w:
                gw = grads[rec.w_i] = z32[o32:o32 + n_out * rec.k_total].view(n_out, rec.k_total)
                o32 += n_out * rec.k_total
                _weight_gradient(rec, gw, gh, xs, g_scr, lambda: _input_rows(recs[si - 1] if si else None, kept, blocks0, m_rows),
                                 gather if si == 0 else None, m_rows)
            if si > 0:
                g = gx
            elif need_x:
                _block_gradients(grads, blocks0, wants, gather, gx)
        if casts:
            c32 = z64.to(torch.float32)
            for gi, o0, n in casts:
                grads[gi] = c32[o0:o0 + n]
        return (None, None, None) + tuple(grads)


def _segment_sum_cols(edge_index, mode, n_nodes, rows, col0, width):
    """sum over the columns e of edge_index with edge_index[mode, e] = v of rows[e, col0 : col0 + width] -> [n_nodes, width]: the input gradient
    of a block gathered through edge_index[mode], read where the input-gradient product left it (gsn_segment_sum_rows_hip: the slice is not
    copied).  Slices that are not 16-byte aligned take the copy + propagate route."""
    E = rows.shape[0]
    if E == 0 or rows.dtype is not torch.float32 or rows.stride(1) != 1 or (col0 | width | rows.stride(0)) % 4 or rows.data_ptr() % 16:
        with torch.no_grad():
            return propagate(0, edge_index, mode, n_nodes, b=rows[:, col0:col0 + width].contiguous())
    csr = _csr_for(edge_index, mode, n_nodes)
    src = edge_index[1 - mode].contiguous()
    out = torch.empty((n_nodes, width), dtype=torch.float32, device=rows.device)
    with _abi.device_guard(rows.device), _timed("propagate_fwd", 12.0 * E + 4.0 * n_nodes + 4.0 * (E + n_nodes) * width):
        rc = _abi.lib().gsn_segment_sum_rows_hip(n_nodes, E, src.data_ptr(), csr.seg_ptr.data_ptr(), csr.perm.data_ptr(),
                                                 csr.src.data_ptr() if csr.src is not None else None, rows.data_ptr() + 4 * col0, width,
                                                 rows.stride(0), out.data_ptr(), _abi.current_stream())
    _abi.check(rc, "gsn_segment_sum_rows_hip")
    return out


class _FoldWeightsFn(torch.autograd.Function):
    """w_first = [W3[:, :d_x] | W3[:, d_x:] W2 | W3[:, d_x:] b2 | pad zero columns]: update_fn's first weight with msg_fn's last Linear (W2, b2) folded in
    (GSN_edge_sparse.py:153-170: update_fn(cat(x, sum_e msg_fn(...)))), differentiable in W3, W2 and b2; one launch each way."""

    @staticmethod
    def takes(w3, last, d_x):
        w2, b2 = last.weight, last.bias
        return (b2 is not None and w3.is_cuda and all(t.dtype is torch.float32 and t.is_contiguous() for t in (w3, w2, b2))
                and w3.shape[1] - d_x == w2.shape[0] and max(w3.shape[0], w2.shape[0], w2.shape[1]) <= 8192
                and w3.shape[0] * w2.shape[0] * w2.shape[1] <= (1 << 25))      # (plain FMA dot products: the matrices of a layer, not a workload)

    @staticmethod
    def forward(ctx, w3, w2, b2, d_x, pad=0):
        R, A, H = w3.shape[0], w2.shape[0], w2.shape[1]
        out = torch.empty((R, d_x + H + 1 + pad), dtype=torch.float32, device=w3.device)
        with _abi.device_guard(w3.device):
            rc = _abi.lib().gsn_fold_weights_fwd_hip(R, d_x, A, H, pad, w3.data_ptr(), w3.stride(0), w2.data_ptr(), w2.stride(0), b2.data_ptr(),
                                                     out.data_ptr(), _abi.current_stream())
        _abi.check(rc, "gsn_fold_weights_fwd_hip")
        ctx.save_for_backward(w3, w2, b2)
        ctx.d_x = d_x
        return out

    @staticmethod
    def backward(ctx, g):
        w3, w2, b2 = ctx.saved_tensors
        d_x, R, A, H = ctx.d_x, w3.shape[0], w2.shape[0], w2.shape[1]
        if g.dtype is not torch.float32 or g.stride(1) != 1:
            g = g.to(torch.float32).contiguous()
        g_w3, g_w2, g_b2 = torch.empty_like(w3), torch.empty_like(w2), torch.empty_like(b2)
        with _abi.device_guard(w3.device):
            rc = _abi.lib().gsn_fold_weights_bwd_hip(R, d_x, A, H, g.data_ptr(), g.stride(0), w3.data_ptr(), w3.stride(0), w2.data_ptr(), w2.stride(0),
                                                     b2.data_ptr(), g_w3.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(), _abi.current_stream())
        _abi.check(rc, "gsn_fold_weights_bwd_hip")
        return g_w3, g_w2, g_b2, None, None


def _dense_native_ok(stages, training=None):
    """Native backward covers: plain (un-gathered) blocks, <= 5 of them; BatchNorm on batch statistics or (r03) on its running
    statistics -- each BatchNorm1d module's own ``training`` flag decides, as in the reference (models_misc.py:41-45)."""
    if not flags.NATIVE_DENSE_BACKWARD or not stages or len(stages[0].blocks) > 5:
        return False
    for i, st in enumerate(stages):
        if any(idx is not None for _, idx in st.blocks) or (i > 0 and st.blocks):
            return False
    return True


def run_stages_autograd(stages, m_rows, training, gather=None, rows=None):
    """Differentiable evaluation of a dense stage list with the native adjoint.  ``gather = (edge_index, n_nodes, modes)``: block b of
    the first stage is gathered through ``edge_index[modes[b]]`` (None: one row per edge) -- the edge rows cat(x_i, x_j, ..) of
    GSN_sparse.py:166-171 are then never assembled, neither for the product nor for the weight gradient.  ``rows``: the row class of the
    stages' rows ("vertex", "edge", "graph"), named by the call site: under loader.masked_training() the BatchNorm stages take the
    statistics of that class's real rows (a stage list with BatchNorm on batch statistics and no ``rows`` is refused there)."""
    bound = None
    if _bound.is_active() and any(st.bn is not None for st in stages):      # (column sums over rows: batch statistics, or gamma / beta gradients)
        bound = _bound.active(rows, "run_stages_autograd")
    if gather is not None and not any(m is not None for m in gather[2]):
        gather = None
    recs, tensors = _layout(stages)
    return _DenseStagesFn.apply(recs, gather, bound, *tensors)


def _transposed_weight(lin):
    key = (lin.weight._version, lin.weight.data_ptr())
    hit = getattr(lin, "_gsn_wt", None)
    if hit is None or hit[0] != key:
        hit = (key, lin.weight.detach().to(torch.float32).t().contiguous())
        lin._gsn_wt = hit
        _note_cache(lin, "_gsn_wt")
    return hit[1]


def _code_stage_segsum(mf, cblocks, csr, m_rows):
    """msg_fn's first stage over Codes blocks + sum per target: gsn_code_stage_fwd_hip.  ``cblocks``: (Codes, int32 row
    index per target-sorted position) in concatenation order.  Returns [n_nodes, d_h] or None if the shape does not fit."""
    L = _abi.lib()
    lin = mf.fc[0]
    bn = mf.bn[0] if mf.batch_norm else None
    n_out, k_total = lin.weight.shape
    n_slots = sum(len(c.n_classes) for c, _ in cblocks)
    if n_slots > 16 or sum(sum(c.n_classes) for c, _ in cblocks) != k_total or not L.gsn_code_stage_supported(n_slots, k_total, n_out):
        return None
    dev = lin.weight.device
    arr = (_abi.gsn_code_slot * n_slots)()
    s, off = 0, 0
    for c, idx in cblocks:
        for col, ncls in enumerate(c.n_classes):
            arr[s].codes = c.codes.data_ptr(); arr[s].idx = idx.data_ptr()
            arr[s].stride = c.codes.shape[1]; arr[s].col = col; arr[s].w_off = off; arr[s].n_classes = ncls
            arr[s].clamp = int(c.clamp)
            s += 1
            off += ncls
    wt = _transposed_weight(lin)
    bias = _f32c(lin.bias)
    status = _zeros(1, torch.int32, dev)

    def launch(bn_params, out, stats):
        vecs = [None if v is None else _f32c(v) for v in (bn_params or (None, None, None))]
        with _abi.device_guard(dev), _timed("code_stage", 4.0 * m_rows * n_slots * n_out):
            rc = L.gsn_code_stage_fwd_hip(m_rows, n_slots, arr, wt.data_ptr(), k_total, bias.data_ptr(), n_out,
                                          _abi.ptr(vecs[0]), _abi.ptr(vecs[1]), _abi.ptr(vecs[2]), _ACT_CODE[mf.activation_name],
                                          csr.tgt.data_ptr(), _abi.ptr(out), _abi.ptr(stats), status.data_ptr(),
                                          _abi.current_stream())
        _abi.check(rc, "gsn_code_stage_fwd_hip")

    stage = _Stage(lin.weight, lin.bias, bn, mf.activation_name)
    if bn is not None and (mf.training or bn.running_mean is None):
        _bound.refuse("_code_stage_segsum (msg_fn's first stage over integer codes)")

    def stats_fn():
        stats = _zeros(2 * n_out, torch.float64, dev).view(2, n_out)
        launch(None, None, stats)
        return stats

    _bn_resolve(stage, stats_fn, m_rows, mf.training)
    n_seg = csr.seg_ptr.numel() - 1
    out = torch.empty((n_seg, n_out), dtype=torch.float32, device=dev)
    with _abi.device_guard(dev), _timed("segsum_prepare"):
        _abi.check(L.gsn_segsum_prepare_hip(n_seg, m_rows, csr.seg_ptr.data_ptr(), csr.tgt.data_ptr(), n_out, out.data_ptr(),
                                            _abi.current_stream()), "gsn_segsum_prepare_hip")
    launch(stage.bn_params, out, None)
    if flags.CODE_STATUS_CHECK and int(status.item()) != 0:
        raise IndexError("a code is outside [0, n_classes) of its column")
    return out


class _GatherCatFn(torch.autograd.Function):
    """cat(x[idx_i], x[idx_j], ids.., e) for the training path (gsn_gather_cat_hip); the adjoint of a gathered block is the
    scatter-add over its index = the propagate kernel on the cached CSR of that edge_index row."""

    @staticmethod
    def forward(ctx, edge_index, n_nodes, modes, *tensors):
        # modes[b]: 0 / 1 = rows gathered through edge_index[0] / edge_index[1], None = one row per edge
        E = edge_index.shape[1]
        ts = [_f32c(t) for t in tensors]
        keep = []
        arr = _block_array([(t, None if m is None else edge_index[m]) for t, m in zip(ts, modes)], keep)
        k_total = sum(t.shape[1] for t in ts)
        out = torch.empty((E, k_total), dtype=torch.float32, device=edge_index.device)
        with _abi.device_guard(out.device), _timed("gather_cat", 8.0 * out.numel()):
            _abi.check(_abi.lib().gsn_gather_cat_hip(E, len(ts), arr, out.data_ptr() if E else None, _abi.current_stream()),
                       "gsn_gather_cat_hip")
        ctx.edge_index, ctx.n_nodes, ctx.modes = edge_index, n_nodes, modes
        ctx.widths = [t.shape[1] for t in ts]
        return out

    @staticmethod
    def backward(ctx, g):
        grads, o = [], 0
        for b, (w, m) in enumerate(zip(ctx.widths, ctx.modes)):
            if not ctx.needs_input_grad[3 + b]:
                grads.append(None)
            else:
                gb = g[:, o:o + w].contiguous()
                # rows gathered through edge_index[m]: sum the per-edge gradients per vertex of that row
                grads.append(gb if m is None else propagate(0, ctx.edge_index, m, ctx.n_nodes, b=gb))
            o += w
        return (None, None, None) + tuple(grads)


class _HipWithTorchBackward(torch.autograd.Function):
    """y = hip_fn() in forward; gradients by re-running a differentiable evaluation of the same function under autograd: the PyTorch
    twin here, a composition of kernels that each have a HIP adjoint in the subclass below (same mechanics)."""

    @staticmethod
    def forward(ctx, hip_fn, torch_fn, n_inputs, *tensors):
        ctx.torch_fn, ctx.n_inputs = torch_fn, n_inputs
        ctx.params = list(tensors[n_inputs:])   # the module's own Parameter objects (the twin reads them directly)
        ctx.save_for_backward(*tensors[:n_inputs])
        with torch.no_grad():
            return hip_fn()

    @staticmethod
    def backward(ctx, gy):
        tensors = ctx.saved_tensors
        ins = [t.detach().requires_grad_(ctx.needs_input_grad[3 + i]) for i, t in enumerate(tensors)]
        params = ctx.params
        with torch.enable_grad():
            y = ctx.torch_fn(*ins)
            wanted = [t for t in ins if t.requires_grad] + [p for i, p in enumerate(params) if ctx.needs_input_grad[3 + ctx.n_inputs + i]]
            grads = torch.autograd.grad(y, wanted, gy, allow_unused=True) if wanted else []
        it = iter(grads)
        out = [None, None, None]
        for t in ins:
            out.append(next(it) if t.requires_grad else None)
        for i, p in enumerate(params):
            out.append(next(it) if ctx.needs_input_grad[3 + ctx.n_inputs + i] else None)
        return tuple(out)


class _HipWithNativeBackward(_HipWithTorchBackward):
    """Same, with ``torch_fn`` a composition of HIP kernels with HIP adjoints (eval-mode gradients: the fused forward keeps nothing,
    the backward re-runs the stages materialised and walks their adjoints -- gsn_bn_act_bwd_hip, gsn_wgrad_hip, gsn_propagate_bwd_hip)."""


def _run(module, hip_fn, torch_fn, inputs, extra_params=(), native=False):
    if not torch.is_grad_enabled():
        return hip_fn()
    params = [p for p in module.parameters()] + list(extra_params)
    need_grad = torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in params))
    if not need_grad:
        with torch.no_grad():
            return hip_fn()
    fn = _HipWithNativeBackward if (native and flags.NATIVE_DENSE_BACKWARD) else _HipWithTorchBackward
    return fn.apply(hip_fn, torch_fn, len(inputs), *inputs, *params)
