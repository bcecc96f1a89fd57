"""Which C-ABI entry points ``run_stages_autograd(...)`` followed by ``.backward()`` calls, in order, pinned per route of the dense-stage autograd
function (plain / epilogue-affine / BatchNorm stages on the bf16x6 and fp16x3 kernels, plane-only outputs and adjoints, presplit rows, the
split-rows pre-pass, gathered stage-0 blocks, row bounds of a padded batch, the refusals) -- and every output and gradient of the same cases against
a float64 PyTorch evaluation.

``_abi.lib()`` is wrapped in the recording proxy of tests/test_layer_routes_gpu.py for the length of a case.  EXPECTED (the entry names) and
PARENT_ERR (the relative errors against float64) were recorded once from commit e51f922, the last one before the dense-stage autograd function
was rewritten around one stage record, with this test code, and are literals: a refactor of the host side must make the same foreign calls in the
same order.  The routes are reached at m = 130 rows and widths 12 -> 136 -> 12 (one full 128 tile + a partial one each way) by lowering the
thresholds in ``gsn_amd.flags``, which are all read at call time."""
import copy
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 130


class _Recorder:
    """Stands in for the ctypes handle ``_abi.lib()`` returns: every entry point called through it is noted by name (``gsn_fingerprint_hip``,
    the asynchronous cache validation paced by the wall clock, is not part of a route and is left out)."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name == "gsn_fingerprint_hip":
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call

    def take(self):
        out, self.names = self.names, []
        return out


def C(name, bn=("train", None), widths=(12, 136, 12), m=M, switches=(), x_grad=True, gather=None, bound=None):
    """bn: per stage None | "train" | "eval" (gamma / beta gradients) | "frozen" (eval mode, gamma / beta without gradients).  Stage i maps
    widths[i] -> widths[i + 1]; every stage but the last ends in relu.  gather: the widths of stage 0's blocks, gathered through
    edge_index[(0, 1, None)] of a 2 x m edge_index over 40 vertices.  bound: "vertex" (row_ptr given) | "graph" (no row_ptr): 97 real rows of m."""
    return dict(name=name, bn=bn, widths=widths, m=m, switches=dict(switches), x_grad=x_grad, gather=gather, bound=bound)


F16 = (("LINEAR_F16X3_MIN_N", 0), ("LINEAR_F16X3_MIN_TILES", 0))      # every product the fp16x3 kernel takes at all runs on it
UNFUSED = (("FUSE_BN_ACT_ROWS", 0),)
N_VERT, REAL = 40, 97

CASES = [
    C("plain_bf16x6", bn=(None, None)),
    C("plain_f16x3", bn=(None, None), switches=F16),
    # (the split-K input-gradient product wants six K slices and more: the smallest hidden width that has them, 136 has five)
    C("plain_splitk", bn=(None, None), widths=(12, 200, 12)),
    C("plain_no_splitk", bn=(None, None), widths=(12, 200, 12), switches=(("LINEAR_SPLITK", False),)),
    C("plain_no_strided", bn=(None, None), switches=(("STRIDED_WEIGHTS", False), ("LINEAR_SPLITK", False))),
    C("affine", bn=("frozen", None)),
    C("affine_f16x3", bn=("frozen", None), switches=F16),
    C("bn_eval_grad", bn=("eval", None)),
    C("bn_eval_grad_f16x3", bn=("eval", None), switches=F16 + UNFUSED),
    C("train_fused"),
    C("train_unfused", switches=UNFUSED),
    C("train_fused_f16x3", switches=F16),
    C("train_planes", switches=F16 + UNFUSED),
    C("train_planes_14", widths=(12, 136, 14), switches=F16 + UNFUSED),
    C("train_planes_off", switches=F16 + UNFUSED + (("BN_ACT_PLANES", False), ("BN_BWD_PLANES", False))),
    C("train_split_rows", switches=F16 + UNFUSED + (("WGRAD_F16X3_SPLIT_ROWS", 0), ("BN_BWD_PLANES", False)), x_grad=False),
    C("train_no_x_grad", switches=F16 + UNFUSED, x_grad=False),
    C("train_wgrad_off", switches=F16 + UNFUSED + (("WGRAD_F16X3", False),)),
    C("train_stats_off", switches=F16 + UNFUSED + (("LINEAR_F16X3_STATS", False),)),
    C("train_two_bn", bn=("train", "train"), switches=F16 + UNFUSED),
    C("gathered", gather=(12, 12, 12)),
    C("gathered_misaligned", gather=(14, 14, 12)),          # (the second block starts at column 14: its gradient by copy + propagate)
    C("gathered_f16x3", gather=(12, 12, 12), switches=F16 + UNFUSED),
    C("bounded_vertex", bound="vertex"),
    C("bounded_graph", bound="graph"),
    C("bounded_f16x3", bound="vertex", switches=F16),
    # (m > 16384 rows and K = 12 <= LINEAR_F16X3_MIN_N: the input-gradient product of stage 0 reads a contiguous transposed copy of W)
    C("transposed_copy", bn=(None, None), m=16400),
    C("no_rows", m=0),
    C("no_rows_plain", bn=(None, None), m=0),
]


def _modules(case, seed=0):
    torch.manual_seed(seed)
    k0 = sum(case["gather"]) if case["gather"] else case["widths"][0]
    dims = (k0,) + tuple(case["widths"][1:])
    lins, bns = [], []
    for i, kind in enumerate(case["bn"]):
        lins.append(torch.nn.Linear(dims[i], dims[i + 1]).to(DEV))
        bn = None
        if kind is not None:
            bn = torch.nn.BatchNorm1d(dims[i + 1]).to(DEV).train(kind == "train")
            with torch.no_grad():
                bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.1)
            if kind == "frozen":
                bn.weight.requires_grad_(False); bn.bias.requires_grad_(False)
        bns.append(bn)
    return lins, bns


def _inputs(case, seed=0):
    """(blocks, edge_index or None, gy) of a case, seeded"""
    g = torch.Generator(DEV).manual_seed(seed + 7)
    m = case["m"]
    if case["gather"]:
        wi, wj, we = case["gather"]
        ei = torch.randint(0, N_VERT, (2, m), device=DEV, generator=g)
        blocks = [torch.randn(N_VERT, wi, device=DEV, generator=g), torch.randn(N_VERT, wj, device=DEV, generator=g),
                  torch.randn(m, we, device=DEV, generator=g)]
    else:
        ei, blocks = None, [torch.randn(m, case["widths"][0], device=DEV, generator=g)]
    gy = torch.randn(m, case["widths"][-1], device=DEV, generator=g)
    if case["bound"]:           # (the masked loss of a padded batch: no gradient comes back into a pad row of the last, unbounded stage)
        gy[REAL:] = 0
    return blocks, ei, gy


def _padded_batch(kind, m):
    """what loader.masked_training reads of a padded batch, over tensors made by hand: REAL real rows of m"""
    if kind == "vertex":        # (n_valid = 3 graphs, ptr[3] = REAL vertices)
        nv, ptr = torch.tensor([3], device=DEV), torch.tensor([0, 30, 60, REAL, m, m], device=DEV)
        return types.SimpleNamespace(padded=True, graph_partition=None, n_valid=nv, ptr=ptr, num_real_graphs=3, num_real_nodes=REAL, num_real_edges=0)
    nv = torch.tensor([REAL], device=DEV)           # (the rows are graphs: n_valid itself, no pointer)
    return types.SimpleNamespace(padded=True, graph_partition=None, n_valid=nv, ptr=torch.arange(m + 1, device=DEV), num_real_graphs=REAL,
                                 num_real_nodes=REAL, num_real_edges=0)


def _native(case, lins, bns, blocks, ei, gy, rec=None, rows=None):
    """the stages on the native path: (y, {name: gradient}), the recorder's names taken after forward and after backward"""
    from gsn_amd import _autograd
    from gsn_amd._dense import _Stage
    n = len(lins)
    for i, b in enumerate(blocks):
        b.requires_grad_(case["x_grad"])
    stages = [_Stage(lins[i].weight, lins[i].bias, bns[i], "relu" if i + 1 < n else "identity", blocks=[(b, None) for b in blocks] if i == 0 else ())
              for i in range(n)]
    gather = (ei, N_VERT, (0, 1, None)) if ei is not None else None
    m = gy.shape[0]
    phases = []
    y = _autograd.run_stages_autograd(stages, m, True, gather=gather, rows=rows)
    if rec is not None:
        phases.append(rec.take())
    (y * gy).sum().backward()
    if rec is not None:
        phases.append(rec.take())
    return y.detach(), _grads(blocks, lins, bns), phases


def _grads(blocks, lins, bns):
    out = {}
    for i, b in enumerate(blocks):
        out["x%d" % i] = b.grad
    for i, (lin, bn) in enumerate(zip(lins, bns)):
        out["W%d" % i], out["b%d" % i] = lin.weight.grad, lin.bias.grad
        if bn is not None:
            out["gamma%d" % i], out["beta%d" % i] = bn.weight.grad, bn.bias.grad
    return {k: v for k, v in out.items() if v is not None}


def _float64(case, lins, bns, blocks, ei, gy, real):
    """the same stages in float64 PyTorch over the first ``real`` rows"""
    lins, bns = copy.deepcopy(lins), copy.deepcopy(bns)
    blocks = [b.detach().double().requires_grad_(case["x_grad"]) for b in blocks]
    if ei is None:
        h = blocks[0][:real]
    else:
        h = torch.cat([blocks[0][ei[0]], blocks[1][ei[1]], blocks[2]], 1)[:real]
    for i, (lin, bn) in enumerate(zip(lins, bns)):
        h = lin.double()(h)
        if bn is not None:
            h = bn.double()(h)
        if i + 1 < len(lins):
            h = torch.relu(h)
    (h * gy[:real].double()).sum().backward()
    return h.detach(), _grads(blocks, lins, bns)


def _rel(a, r, scale=None):
    scale = r.abs().max().item() if scale is None else scale
    return 0.0 if r.numel() == 0 else (a.double() - r).abs().max().item() / max(scale, 1e-300)


def _scale(k, case, g64):
    """The magnitude an error of gradient ``k`` is measured against: the tensor's own largest magnitude -- but a bias in front of a train-mode
    BatchNorm has the exact gradient 0 (a column sum of gH, whose terms cancel), so its error is measured against the column sums of the same
    rows that do not cancel, the gradients of that stage's gamma and beta."""
    if k[0] == "b" and k[1:].isdigit() and case["bn"][int(k[1:])] == "train":
        return max(g64["gamma" + k[1:]].abs().max().item(), g64["beta" + k[1:]].abs().max().item())
    return None


@functools.lru_cache(maxsize=None)
def run_case(name):
    """(phases, {tensor: relative error against float64}, extras) of one case, run once for every test that reads it"""
    from gsn_amd import _abi, _bound, flags
    case = next(c for c in CASES if c["name"] == name)
    saved = {k: getattr(flags, k) for k in case["switches"]}
    real_lib = _abi.lib()
    rec = _Recorder(real_lib)
    extras = {}
    try:
        for k, v in case["switches"].items():
            setattr(flags, k, v)
        lins, bns = _modules(case)
        blocks, ei, gy = _inputs(case)
        n_real = REAL if case["bound"] else case["m"]
        y64, g64 = _float64(case, lins, bns, blocks, ei, gy, n_real) if case["m"] else (None, None)
        if case["bound"]:          # (the unpadded run of the real rows on modules of their own: its running statistics)
            lins_u, bns_u = copy.deepcopy(lins), copy.deepcopy(bns)
            _native(case, lins_u, bns_u, [b.detach()[:n_real].clone() for b in blocks], None, gy[:n_real])
            extras["running_unpadded"] = [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in bns_u if bn is not None]
        torch.cuda.synchronize()
        _abi._lib = rec
        if case["bound"]:
            with _bound.masked_training(_padded_batch(case["bound"], case["m"])):
                y, g, phases = _native(case, lins, bns, blocks, ei, gy, rec, rows=case["bound"])
        else:
            y, g, phases = _native(case, lins, bns, blocks, ei, gy, rec)
        torch.cuda.synchronize()
    finally:
        _abi._lib = real_lib
        for k, v in saved.items():
            setattr(flags, k, v)
    if not case["m"]:              # (no rows: torch's BatchNorm refuses them in train mode; every gradient is zero, the error is its magnitude)
        assert y.shape == (0, case["widths"][-1])
        return [" ".join(p) for p in phases], {k: v.abs().max().item() if v.numel() else 0.0 for k, v in g.items()}, {"finite": True}
    assert set(g) == set(g64), (sorted(g), sorted(g64))
    errs = {"y": _rel(y[:n_real], y64)}
    errs.update({k: _rel(g[k][:n_real] if k == "x0" else g[k], g64[k][:n_real] if k == "x0" else g64[k], _scale(k, case, g64)) for k in sorted(g)})
    if case["bound"]:
        extras["x_grad_pad"] = g["x0"][n_real:]
        extras["running"] = [(bn.running_mean, bn.running_var, int(bn.num_batches_tracked)) for bn in bns if bn is not None]
    extras["finite"] = all(bool(torch.isfinite(t).all()) for t in [y, *g.values()])
    return [" ".join(p) for p in phases], errs, extras


# Recorded on the parent commit (see the module docstring): one string per forward / backward of the case ...
EXPECTED = {
    "plain_bf16x6": [
        "gsn_linear_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "plain_f16x3": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip gsn_linear_f16x3_kpad "
        "gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_linear_f16x3_fwd_hip gsn_wgrad_f16x3_hip",
    ],
    "plain_splitk": [
        "gsn_linear_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_splitk_hip gsn_wgrad_hip",
    ],
    "plain_no_splitk": [
        "gsn_linear_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "plain_no_strided": [
        "gsn_linear_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_fwd_hip gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_linear_fwd_hip gsn_wgrad_hip",
    ],
    "affine": [
        "gsn_linear_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "affine_f16x3": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip gsn_linear_f16x3_kpad "
        "gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_linear_f16x3_fwd_hip gsn_wgrad_f16x3_hip",
    ],
    "bn_eval_grad": [
        "gsn_linear_fwd_hip gsn_bn_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "bn_eval_grad_f16x3": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_bn_act_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_bwd_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip "
        "gsn_linear_f16x3_fwd_presplit_hip gsn_wgrad_f16x3_hip",
    ],
    "train_fused": [
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "train_unfused": [
        "gsn_linear_fwd_hip gsn_bn_finalize_count_hip gsn_bn_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "train_fused_f16x3": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_act_hip "
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_bwd_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip "
        "gsn_linear_f16x3_fwd_presplit_hip gsn_wgrad_f16x3_hip",
    ],
    "train_planes": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_bwd_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip "
        "gsn_linear_f16x3_fwd_presplit_hip gsn_wgrad_f16x3_hip",
    ],
    "train_planes_14": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_bn_act_hip gsn_wgrad_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_bn_act_bwd_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_fwd_presplit_hip gsn_wgrad_f16x3_hip",
    ],
    "train_planes_off": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_bn_act_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_from_h_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_linear_f16x3_fwd_hip gsn_wgrad_f16x3_hip",
    ],
    "train_split_rows": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_from_h_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_split_rows_hip gsn_wgrad_f16x3_hip",
    ],
    "train_no_x_grad": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_bwd_planes_hip gsn_wgrad_f16x3_hip",
    ],
    "train_wgrad_off": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_bn_act_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_linear_f16x3_fwd_hip gsn_wgrad_hip",
    ],
    "train_stats_off": [
        "gsn_linear_fwd_hip gsn_bn_finalize_count_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad "
        "gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_from_h_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_linear_f16x3_fwd_hip gsn_wgrad_hip",
    ],
    "train_two_bn": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip gsn_bn_finalize_count_hip "
        "gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip "
        "gsn_linear_f16x3_fwd_stats_presplit_hip gsn_bn_finalize_count_hip gsn_bn_act_hip",
        "gsn_linear_f16x3_scratch_bytes gsn_bn_act_bwd_planes_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip "
        "gsn_linear_f16x3_fwd_presplit_hip gsn_wgrad_f16x3_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_bwd_planes_hip gsn_linear_f16x3_kpad "
        "gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_fwd_presplit_hip gsn_wgrad_f16x3_hip",
    ],
    "gathered": [
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems "
        "gsn_csr_build_hip gsn_segment_sum_rows_hip",
    ],
    "gathered_misaligned": [
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_csr_scratch_elems "
        "gsn_csr_build_hip gsn_propagate_self_fwd_hip",
    ],
    "gathered_f16x3": [
        "gsn_linear_fwd_hip gsn_bn_finalize_count_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad "
        "gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_from_h_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes "
        "gsn_linear_f16x3_fwd_hip gsn_wgrad_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems "
        "gsn_csr_build_hip gsn_segment_sum_rows_hip",
    ],
    "bounded_vertex": [
        "gsn_linear_fwd_hip gsn_bn_finalize_bounded_scratch_bytes gsn_bn_finalize_bounded_hip gsn_bn_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_bounded_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "bounded_graph": [
        "gsn_linear_fwd_hip gsn_bn_finalize_bounded_scratch_bytes gsn_bn_finalize_bounded_hip gsn_bn_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_bounded_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip",
    ],
    "bounded_f16x3": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_stats_hip "
        "gsn_bn_finalize_bounded_scratch_bytes gsn_bn_finalize_bounded_hip gsn_linear_f16x3_scratch_bytes gsn_bn_act_planes_hip gsn_linear_f16x3_kpad "
        "gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_fwd_presplit_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_f16x3_hip gsn_bn_act_bwd_from_h_bounded_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip "
        "gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip gsn_wgrad_f16x3_hip",
    ],
    "transposed_copy": [
        "gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_f16x3_kpad gsn_linear_f16x3_prepare_strided_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_fwd_hip "
        "gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_hip gsn_linear_f16x3_scratch_bytes gsn_linear_f16x3_split_rows_hip "
        "gsn_wgrad_f16x3_hip",
    ],
    "no_rows": [
        "gsn_bn_act_hip",
        "gsn_bn_act_bwd_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_wgrad_hip",
    ],
    "no_rows_plain": [
        "",
        "gsn_bn_act_bwd_hip gsn_wgrad_hip gsn_bn_act_bwd_hip gsn_wgrad_hip",
    ],
}

# ... and the parent's relative errors (max |got - float64| / max |float64|) of the output and every gradient.
PARENT_ERR = {
    "plain_bf16x6": {"y": 2.9e-07, "W0": 2.67e-07, "W1": 2.53e-07, "b0": 1.69e-07, "b1": 3.05e-08, "x0": 3.16e-07},
    "plain_f16x3": {"y": 2.73e-07, "W0": 2.33e-07, "W1": 2.2e-07, "b0": 1.46e-07, "b1": 3.05e-08, "x0": 2.26e-07},
    "plain_splitk": {"y": 2.58e-07, "W0": 2.16e-07, "W1": 1.77e-07, "b0": 1.3e-07, "b1": 3.05e-08, "x0": 2.41e-07},
    "plain_no_splitk": {"y": 2.58e-07, "W0": 2.16e-07, "W1": 1.77e-07, "b0": 1.3e-07, "b1": 3.05e-08, "x0": 2.59e-07},
    "plain_no_strided": {"y": 2.9e-07, "W0": 2.17e-07, "W1": 2.53e-07, "b0": 1.69e-07, "b1": 3.05e-08, "x0": 3.16e-07},
    "affine": {"y": 4.74e-07, "W0": 1.54e-07, "W1": 1.63e-07, "b0": 9.82e-08, "b1": 3.05e-08, "x0": 2.48e-07},
    "affine_f16x3": {"y": 2.69e-07, "W0": 1.55e-07, "W1": 1.8e-07, "b0": 1.09e-07, "b1": 3.05e-08, "x0": 2.39e-07},
    "bn_eval_grad": {"y": 4.74e-07, "W0": 1.57e-07, "W1": 1.63e-07, "b0": 9.82e-08, "b1": 3.05e-08, "beta0": 1.53e-07, "gamma0": 2.39e-07, "x0":
        2.48e-07},
    "bn_eval_grad_f16x3": {"y": 2.69e-07, "W0": 1.55e-07, "W1": 1.8e-07, "b0": 9.65e-08, "b1": 3.05e-08, "beta0": 1.17e-07, "gamma0": 2.15e-07, "x0":
        2.39e-07},
    "train_fused": {"y": 3.23e-07, "W0": 1.56e-07, "W1": 2.31e-07, "b0": 1.49e-07, "b1": 3.05e-08, "beta0": 9.76e-08, "gamma0": 1.47e-07, "x0":
        2.49e-07},
    "train_unfused": {"y": 3.23e-07, "W0": 1.46e-07, "W1": 2.31e-07, "b0": 1.49e-07, "b1": 3.05e-08, "beta0": 9.76e-08, "gamma0": 1.47e-07, "x0":
        2.49e-07},
    "train_fused_f16x3": {"y": 2.44e-07, "W0": 2.04e-07, "W1": 1.69e-07, "b0": 5.6e-16, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.86e-07, "x0":
        2.07e-07},
    "train_planes": {"y": 2.44e-07, "W0": 2.04e-07, "W1": 1.69e-07, "b0": 5.6e-16, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.86e-07, "x0":
        2.07e-07},
    "train_planes_14": {"y": 2.54e-07, "W0": 2.44e-07, "W1": 1.77e-07, "b0": 4.32e-16, "b1": 3.4e-08, "beta0": 1.24e-07, "gamma0": 1.45e-07, "x0":
        2.16e-07},
    "train_planes_off": {"y": 2.44e-07, "W0": 2.04e-07, "W1": 1.69e-07, "b0": 1.39e-07, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.86e-07, "x0":
        2.07e-07},
    "train_split_rows": {"y": 2.44e-07, "W0": 2.04e-07, "W1": 1.69e-07, "b0": 1.39e-07, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.86e-07},
    "train_no_x_grad": {"y": 2.44e-07, "W0": 2.04e-07, "W1": 1.69e-07, "b0": 5.6e-16, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.86e-07},
    "train_wgrad_off": {"y": 2.44e-07, "W0": 2.08e-07, "W1": 2.34e-07, "b0": 1.39e-07, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.86e-07, "x0":
        2.07e-07},
    "train_stats_off": {"y": 2.44e-07, "W0": 1.63e-07, "W1": 1.9e-07, "b0": 1.56e-07, "b1": 3.05e-08, "beta0": 1.12e-07, "gamma0": 1.8e-07, "x0":
        2.41e-07},
    "train_two_bn": {"y": 3.19e-07, "W0": 3.01e-07, "W1": 2.7e-07, "b0": 8.3e-16, "b1": 1.25e-15, "beta0": 1.95e-07, "beta1": 3.05e-08, "gamma0":
        2.11e-07, "gamma1": 3.79e-07, "x0": 1.93e-07},
    "gathered": {"y": 3.59e-07, "W0": 2.73e-07, "W1": 2.17e-07, "b0": 1.64e-07, "b1": 3.89e-08, "beta0": 1.47e-07, "gamma0": 1.92e-07, "x0": 2.45e-07,
        "x1": 2.83e-07, "x2": 3.98e-07},
    "gathered_misaligned": {"y": 2.99e-07, "W0": 1.26e-07, "W1": 1.74e-07, "b0": 1.54e-07, "b1": 3.89e-08, "beta0": 8.58e-08, "gamma0": 1.69e-07,
        "x0": 1.77e-07, "x1": 2.39e-07, "x2": 2.9e-07},
    "gathered_f16x3": {"y": 2.18e-07, "W0": 2.41e-07, "W1": 2.17e-07, "b0": 1.98e-07, "b1": 3.89e-08, "beta0": 1.5e-07, "gamma0": 2.02e-07, "x0":
        1.98e-07, "x1": 2.3e-07, "x2": 2.14e-07},
    "bounded_vertex": {"y": 5.19e-07, "W0": 1.53e-07, "W1": 2.27e-07, "b0": 1.39e-07, "b1": 2.27e-08, "beta0": 1.15e-07, "gamma0": 1.04e-07, "x0":
        2.04e-07},
    "bounded_graph": {"y": 5.19e-07, "W0": 1.53e-07, "W1": 2.27e-07, "b0": 1.39e-07, "b1": 2.27e-08, "beta0": 1.15e-07, "gamma0": 1.04e-07, "x0":
        2.04e-07},
    "bounded_f16x3": {"y": 2.68e-07, "W0": 1.59e-07, "W1": 2.21e-07, "b0": 1.23e-07, "b1": 2.27e-08, "beta0": 9.12e-08, "gamma0": 1.57e-07, "x0":
        2.14e-07},
    "transposed_copy": {"y": 3.45e-07, "W0": 3.88e-07, "W1": 3.96e-07, "b0": 7.14e-07, "b1": 3.93e-08, "x0": 4.05e-07},
    "no_rows": {"x0": 0, "W0": 0, "b0": 0, "gamma0": 0, "beta0": 0, "W1": 0, "b1": 0},
    "no_rows_plain": {"x0": 0, "W0": 0, "b0": 0, "W1": 0, "b1": 0},
}


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_stage_list_makes_the_recorded_foreign_calls(name):
    phases, errs, extras = run_case(name)
    print(name, phases)
    assert phases == EXPECTED[name]
    assert extras["finite"]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_outputs_and_gradients_match_float64(name):
    """every output and gradient within max(2 x the parent's error on that case and tensor, 2e-6) of float64, relative to the tensor's largest
    magnitude (the rule of tests/test_wgrad16_gpu.py; the factor 2: float atomics in the weight-gradient and split-k sums reorder from run to run)"""
    phases, errs, extras = run_case(name)
    print(name, errs)
    assert set(errs) == set(PARENT_ERR[name])
    for k, e in errs.items():
        assert e <= max(2.0 * PARENT_ERR[name][k], 2e-6), (name, k, e, PARENT_ERR[name][k])


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["bound"]])
def test_bounded_stage_leaves_pad_rows_zero_and_counts_real_rows(name):
    """gX = gH W of the bounded stage 0: its pad rows are exactly +0 only if gH's are; the running statistics are those of the real rows"""
    phases, errs, extras = run_case(name)
    pad = extras["x_grad_pad"]
    assert pad.shape[0] == M - REAL and bool((pad == 0).all()) and not bool(torch.signbit(pad).any())
    assert "gsn_bn_finalize_bounded_hip" in phases[0] and "gsn_bn_act_bwd_from_h_bounded_hip" in phases[1]
    for (mean, var, nbt), (mean_u, var_u, nbt_u) in zip(extras["running"], extras["running_unpadded"]):
        assert nbt == nbt_u == 1
        assert _rel(mean, mean_u.double()) <= 1e-6 and _rel(var, var_u.double()) <= 1e-6


def test_refusals_keep_their_texts():
    from gsn_amd import _abi, _bound
    case = C("refusals")
    lins, bns = _modules(case)
    blocks, ei, gy = _inputs(case)
    with _bound.masked_training(_padded_batch("vertex", M)):
        with pytest.raises(RuntimeError) as e:
            _native(case, lins, bns, blocks, ei, gy)
    assert str(e.value) == ("run_stages_autograd: train-mode BatchNorm statistics under loader.masked_training() on a path that does not name its "
                            "row class (the statistics would run over the pad rows)")
    one = _padded_batch("graph", M)
    one.n_valid.fill_(1); one.num_real_graphs = 1
    with _bound.masked_training(one):
        with pytest.raises(ValueError) as e:
            _native(case, lins, bns, blocks, ei, gy, rows="graph")
    assert str(e.value) == "Expected more than 1 value per channel when training, got input size torch.Size([1, 136])"
    assert not _bound.is_active()


def test_one_row_in_train_mode_is_refused_in_torch_s_words():
    case = C("one_row", m=1)
    lins, bns = _modules(case)
    blocks, ei, gy = _inputs(case)
    with pytest.raises(ValueError) as theirs:
        bns[0](lins[0](blocks[0]))
    with pytest.raises(ValueError) as ours:
        _native(case, lins, bns, blocks, ei, gy)
    assert str(ours.value) == str(theirs.value)


def test_table_covers_every_arm():
    """The recorded table itself: between them the cases call every entry the dense-stage autograd function chooses among."""
    seen = set(" ".join(" ".join(p) for p in EXPECTED.values()).split())
    for entry in ("gsn_linear_fwd_hip", "gsn_linear_fwd_strided_hip", "gsn_linear_fwd_splitk_hip", "gsn_linear_f16x3_fwd_hip", "gsn_linear_f16x3_fwd_stats_hip",
                  "gsn_linear_f16x3_fwd_presplit_hip", "gsn_linear_f16x3_split_rows_hip", "gsn_bn_finalize_count_hip", "gsn_bn_finalize_act_hip",
                  "gsn_bn_finalize_bounded_hip", "gsn_bn_act_hip", "gsn_bn_act_planes_hip", "gsn_bn_act_bwd_hip", "gsn_bn_act_bwd_from_h_hip",
                  "gsn_bn_act_bwd_from_h_bounded_hip", "gsn_bn_act_bwd_planes_hip", "gsn_wgrad_hip", "gsn_wgrad_f16x3_hip", "gsn_segment_sum_rows_hip"):
        assert entry in seen, entry
    assert set(EXPECTED) == set(PARENT_ERR) == {c["name"] for c in CASES}
