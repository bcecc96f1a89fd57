"""Which C-ABI entry points one layer forward calls, in order, pinned per route of ``_SparseLayer._hip`` (recorded launch, code packs, code-stage
gather, one-launch kernel, split edge stage, chain + segment sum, materialised rows, the gin / ogb arm, the training compositions).

``_abi.lib()`` is wrapped in a recording proxy for the duration of a case; nothing in the library changes.  The EXPECTED table was recorded once
from commit e2cc405, the last one before the layers were rewritten around one message-row layout, and is a literal: a refactor of the host
side must make the same foreign calls in the same order.  ``gsn_fingerprint_hip`` (the asynchronous cache validation in front of
``_hip``, paced by the wall clock) is not part of a route and is left out of the record."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _Recorder:
    """Stands in for the ctypes handle ``_abi.lib()`` returns: every entry point called through it is noted by name."""

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


def C(name, cls, x, ids=None, ef=None, scope=None, d=64, d_h=None, act="relu", bn=True, kind="general", flow="source_to_target",
      mode="eval", calls=1, switches=(), partition=False, post=False, tagged=False, edgeless=False):
    """x / ids / ef: an int = dense fp32 rows of that width, a list = layers.Codes with those class counts (``tagged``: their dense one-hot
    rows, tagged with exact fp16 packs).  mode: eval | eval_grad | train | train_nograd.  switches: ((flag name, value), ...)."""
    return dict(name=name, cls=cls, x=x, ids=ids, ef=ef, scope=scope, d=d, d_h=[d] if d_h is None else d_h, act=act, bn=bn, kind=kind, flow=flow,
                mode=mode, calls=calls, switches=dict(switches), partition=partition, post=post, tagged=tagged, edgeless=edgeless)


OFF_FUSED = (("FUSED_LAYER", False),)
OFF_BOTH = (("FUSED_LAYER", False), ("SPLIT_EDGE_STAGE", False))
GIN = dict(kind="gin")

CASES = [
    # integer codes in, eval: the packed-row kernel on packs made from the codes; the second forward is the recorded launch
    C("codes_pack", "GSN_edge_sparse", [28], [3, 3, 3, 3], [4], "local", d=128, calls=2),
    C("codes_pack_mpnn_edge", "MPNN_edge_sparse", [28], None, [4], d=128, calls=2),
    C("codes_pack_t2s", "GSN_sparse", [5], [3, 4], None, "local", d=128, flow="target_to_source"),
    # codes outside the packs (too wide, global scope, an activation the one-launch kernel does not take, the switch off): weight-row gather
    C("codes_gather_wide", "GSN_edge_sparse", [28], [3, 4, 4, 5], [4], "local", d=128),
    C("codes_gather_global", "GSN_edge_sparse", [28], [3, 4, 4, 5, 2, 2], [4], "global", d=128),
    C("codes_gather_elu", "GSN_edge_sparse", [9, 3], [7], [4, 2], "local", d=64, act="elu", bn=False, flow="target_to_source"),
    C("codes_gather_pack16_off", "GSN_edge_sparse", [28], [3, 3, 3, 3], [4], "local", d=128, switches=(("PACK16_LAYER", False),)),
    C("codes_gather_train_nograd", "GSN_edge_sparse", [28], [3, 4], [4], "local", d=64, mode="train_nograd"),
    # ... and codes the gather stage declines (18 slots): dense one-hot rows after all
    C("codes_declined", "GSN_sparse", [5], [2] * 17, None, "local", d=64),
    # dense inputs: the one-launch kernels
    C("fused_rows", "GSN_edge_sparse", 28, 12, 4, "local", d=64, calls=2),
    C("fused_rows_mpnn", "MPNN_sparse", 32, d=64),
    C("fused_rows_post", "MPNN_edge_sparse", 28, None, 4, d=64, post=True),
    C("fused_rows_global", "GSN_sparse", 16, 8, None, "global", d=64),
    C("fused_tagged", "GSN_edge_sparse", [28], [3, 3, 3, 3], [4], "local", d=128, calls=2, tagged=True),
    C("wide_graphs", "GSN_edge_sparse", 128, 12, 4, "local", d=128, calls=2, partition=True, post=True),
    C("wide_rows", "GSN_edge_sparse", 128, 12, 4, "local", d=128, calls=2),
    # the one-launch kernel switched off: split edge stage (K > 160), chain + segment sum, materialised rows + propagate
    C("split_edge", "GSN_edge_sparse", 128, 12, 4, "local", d=128, switches=OFF_FUSED),
    C("split_edge_global", "GSN_edge_sparse", 64, 24, 4, "global", d=64, switches=OFF_FUSED),
    C("chain_segsum", "GSN_edge_sparse", 28, 12, 4, "local", d=64, switches=OFF_BOTH),
    C("chain_segsum_global", "GSN_sparse", 16, 8, None, "global", d=64, switches=OFF_BOTH, flow="target_to_source"),
    C("materialised", "GSN_edge_sparse", 28, 7, 4, "local", d=200, act="tanh", switches=OFF_BOTH),
    C("three_stage_msg", "GSN_edge_sparse", 28, 12, 4, "local", d=64, d_h=[64, 64]),
    C("single_linear_msg", "GSN_edge_sparse", 28, 12, 4, "local", d=64, d_h=[]),
    C("edgeless", "GSN_edge_sparse", 28, 12, 4, "local", d=64, edgeless=True),
    # gin / ogb
    C("gin_local", "GSN_edge_sparse", 28, 7, 4, "local", d=32, **GIN),
    C("gin_global", "GSN_sparse", 28, 7, None, "global", d=32, **GIN),
    C("gin_mpnn_edge", "MPNN_edge_sparse", 28, None, 4, d=32, **GIN),
    C("ogb_gsn_local", "GSN_edge_sparse_ogb", 32, 32, 32, "local", d=32, kind="ogb"),
    C("ogb_gsn_global", "GSN_edge_sparse_ogb", 32, 32, 32, "global", d=32, kind="ogb"),
    C("ogb_mpnn", "MPNN_edge_sparse_ogb", 32, None, 32, d=32, kind="ogb"),
    # train mode (forward, then backward) and eval mode with a gradient asked for
    C("train_general", "GSN_edge_sparse", 28, 12, 4, "local", d=64, mode="train"),
    C("train_general_global", "GSN_sparse", 16, 8, None, "global", d=64, mode="train", flow="target_to_source"),
    C("train_single_linear", "MPNN_sparse", 16, d=32, d_h=[], mode="train"),
    C("train_codes", "GSN_edge_sparse", [28], [3, 4], [4], "local", d=64, mode="train"),
    C("train_gin", "GSN_edge_sparse", 28, 7, 4, "local", d=32, mode="train", **GIN),
    C("train_ogb", "GSN_edge_sparse_ogb", 32, 32, 32, "local", d=32, kind="ogb", mode="train"),
    C("eval_grad_general", "GSN_edge_sparse", 28, 12, 4, "local", d=64, mode="eval_grad"),
    C("eval_grad_global", "GSN_edge_sparse", 28, 12, 4, "global", d=64, mode="eval_grad"),
    C("eval_grad_gin", "GSN_sparse", 28, 7, None, "global", d=32, mode="eval_grad", **GIN),
    C("twin_general", "GSN_edge_sparse", 28, 12, 4, "global", d=64, mode="train", switches=(("NATIVE_DENSE_BACKWARD", False),)),
]


def _width(v):
    return 0 if v is None else (v if isinstance(v, int) else sum(v))


def _build(case, seed=0):
    """(layer, edge_index, x, kwargs) of a case: everything made before the record starts."""
    from gsn_amd import layers, packs, synth
    rng = np.random.default_rng(seed + 11)
    torch.manual_seed(seed)
    if case["edgeless"]:
        n, ei, b = 7, torch.zeros((2, 0), dtype=torch.int64, device=DEV), None
    else:
        b = synth.zinc_shape_batch(12, seed=seed + 3)
        n, ei = b.num_nodes, torch.from_numpy(b.edge_index).to(DEV)
    E = ei.shape[1]
    kw = dict(d_in=_width(case["x"]), d_degree=1, degree_as_tag=False, retain_features=True, d_msg=case["d"], d_up=case["d"], d_h=list(case["d_h"]),
              seed=seed, activation_name=case["act"], bn=case["bn"], msg_kind=case["kind"], flow=case["flow"])
    if case["ids"] is not None:
        kw.update(d_id=_width(case["ids"]), id_scope=case["scope"])
    if case["ef"] is not None:
        kw.update(d_ef=_width(case["ef"]))
    if case["kind"] == "gin":
        kw.update(id_embedding="one_hot_encoder", edge_embedding="one_hot_encoder", extend_dims=True)
    layer = getattr(layers, case["cls"])(**kw).to(DEV)
    layer.train(case["mode"] in ("train", "train_nograd"))
    for m in layer.modules():                  # (running statistics other than 0 / 1: an eval-mode BatchNorm that does something)
        if isinstance(m, torch.nn.BatchNorm1d):
            with torch.no_grad():
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)

    def value(spec, rows):
        if spec is None:
            return None
        if isinstance(spec, int):
            return torch.randn(rows, spec, device=DEV)
        codes = layers.Codes(torch.from_numpy(rng.integers(0, spec, size=(rows, len(spec)))).to(DEV), spec)
        return codes.dense().clone() if case["tagged"] else codes

    x = value(case["x"], n)
    ids = value(case["ids"], E if case["scope"] == "local" else n)
    ef = value(case["ef"], E)
    if case["tagged"]:
        packs.node_pack(x)
        packs.edge_pack([ids, ef])
    if case["partition"]:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        layers.set_graph_partition(ei, t(b.node_ptr), t(b.edge_ptr), int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max()), check=True)
    call = dict(identifiers=ids, degrees=None, edge_features=ef)
    if case["post"]:
        post_bn = torch.nn.BatchNorm1d(case["d"]).to(DEV).train(layer.training)
        with torch.no_grad():
            post_bn.running_mean.normal_(0, 0.1); post_bn.running_var.uniform_(0.5, 1.5)
        call.update(post_bn=post_bn, post_act="relu")
    return layer, ei, x, call


def run_case(case, seed=0):
    """([entry-point names of each forward / backward], [output tensors]) of one case."""
    from gsn_amd import _abi, flags
    saved = {k: getattr(flags, k) for k in case["switches"]}
    real = _abi.lib()
    rec = _Recorder(real)
    phases, outs = [], []
    try:
        for k, v in case["switches"].items():
            setattr(flags, k, v)
        layer, ei, x, call = _build(case, seed)
        torch.cuda.synchronize()
        _abi._lib = rec
        mode = case["mode"]
        if mode in ("eval", "train_nograd"):
            for _ in range(case["calls"]):
                with torch.no_grad():
                    outs.append(layer(x, ei, **call))
                phases.append(rec.take())
        else:
            if isinstance(x, torch.Tensor):
                x.requires_grad_(True)
            y = layer(x, ei, **call)
            phases.append(rec.take())
            gy = torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
            (y * gy).sum().backward()
            phases.append(rec.take())
            outs.append(y.detach())
            if isinstance(x, torch.Tensor):
                outs.append(x.grad)
            outs.extend(p.grad for _, p in sorted(layer.named_parameters()) if p.grad is not None)
        torch.cuda.synchronize()
    finally:
        _abi._lib = real
        for k, v in saved.items():
            setattr(flags, k, v)
    return phases, outs


def digest(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# Recorded on the parent commit (see the module docstring); one string per forward / backward of the case.
EXPECTED = {
    "codes_pack": [
        "gsn_one_hot_pack16_hip gsn_one_hot_pack16_hip gsn_one_hot_pack16_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip "
        "gsn_linear_fwd_hip gsn_layer_fused_pack16_supported gsn_layer_fused_pack16_prepared_bytes gsn_layer_fused_pack16_prepare_hip "
        "gsn_layer_fused_fwd_pack16_hip",
        "gsn_layer_fused_fwd_pack16_hip",
    ],
    "codes_pack_mpnn_edge": [
        "gsn_one_hot_pack16_hip gsn_one_hot_pack16_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip "
        "gsn_layer_fused_pack16_supported gsn_layer_fused_pack16_prepared_bytes gsn_layer_fused_pack16_prepare_hip gsn_layer_fused_fwd_pack16_hip",
        "gsn_layer_fused_fwd_pack16_hip",
    ],
    "codes_pack_t2s": [
        "gsn_one_hot_pack16_hip gsn_one_hot_pack16_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip "
        "gsn_layer_fused_pack16_supported gsn_one_hot_hip gsn_code_stage_supported gsn_segsum_prepare_hip gsn_code_stage_fwd_hip "
        "gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "codes_gather_wide": [
        "gsn_one_hot_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_code_stage_supported gsn_segsum_prepare_hip gsn_code_stage_fwd_hip "
        "gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "codes_gather_global": [
        "gsn_one_hot_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_code_stage_supported gsn_segsum_prepare_hip gsn_code_stage_fwd_hip "
        "gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "codes_gather_elu": [
        "gsn_one_hot_pack16_hip gsn_one_hot_pack16_hip gsn_one_hot_pack16_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip "
        "gsn_linear_fwd_hip gsn_one_hot_hip gsn_code_stage_supported gsn_segsum_prepare_hip gsn_code_stage_fwd_hip gsn_mlp_chain_supported "
        "gsn_mlp_chain_supported gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "codes_gather_pack16_off": [
        "gsn_one_hot_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_code_stage_supported gsn_segsum_prepare_hip gsn_code_stage_fwd_hip "
        "gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "codes_gather_train_nograd": [
        "gsn_one_hot_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_code_stage_supported gsn_code_stage_fwd_hip gsn_bn_finalize_count_hip "
        "gsn_segsum_prepare_hip gsn_code_stage_fwd_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported "
        "gsn_mlp_chain_fwd_hip gsn_bn_finalize_count_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "codes_declined": [
        "gsn_one_hot_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_one_hot_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported "
        "gsn_mlp_chain_supported gsn_mlp_chain_supported gsn_segsum_prepare_hip gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "fused_rows": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
        "gsn_layer_fused_supported gsn_layer_fused_prepared_bytes gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
    ],
    "fused_rows_mpnn": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
    ],
    "fused_rows_post": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
    ],
    "fused_rows_global": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
    ],
    "fused_tagged": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_pack16_supported "
        "gsn_layer_fused_pack16_prepared_bytes gsn_layer_fused_pack16_prepare_hip gsn_layer_fused_fwd_pack16_hip",
        "gsn_layer_fused_fwd_pack16_hip",
    ],
    "wide_graphs": [
        "gsn_csr_build_graphs_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_graphs_supported gsn_layer_fused_fwd_graphs_hip",
        "gsn_layer_fused_fwd_graphs_hip",
    ],
    "wide_rows": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
        "gsn_layer_fused_supported gsn_layer_fused_prepared_bytes gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
    ],
    "split_edge": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_edge_split_sum_hip "
        "gsn_mlp_chain_supported gsn_mlp_chain_supported gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "split_edge_global": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_edge_split_sum_hip "
        "gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "chain_segsum": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported "
        "gsn_segsum_prepare_hip gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "chain_segsum_global": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported "
        "gsn_segsum_prepare_hip gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "materialised": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported "
        "gsn_linear_fwd_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported gsn_linear_fwd_hip gsn_mlp_chain_supported "
        "gsn_linear_fwd_hip",
    ],
    "three_stage_msg": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported "
        "gsn_segsum_prepare_hip gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "single_linear_msg": [
        "gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported "
        "gsn_mlp_chain_fwd_hip",
    ],
    "edgeless": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported "
        "gsn_mlp_chain_fwd_hip",
    ],
    "gin_local": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "gin_global": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "gin_mpnn_edge": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "ogb_gsn_local": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "ogb_gsn_global": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "ogb_mpnn": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
    ],
    "train_general": [
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_fold_weights_fwd_hip "
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_fold_weights_bwd_hip gsn_propagate_pad_bwd_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_segment_sum_rows_hip",
    ],
    "train_general_global": [
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_fold_weights_fwd_hip "
        "gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_fold_weights_bwd_hip gsn_propagate_pad_bwd_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_segment_sum_rows_hip",
    ],
    "train_single_linear": [
        "gsn_linear_fwd_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_propagate_pad_bwd_hip gsn_bn_act_bwd_hip "
        "gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems gsn_csr_build_hip "
        "gsn_segment_sum_rows_hip",
    ],
    "train_codes": [
        "gsn_one_hot_hip gsn_one_hot_hip gsn_one_hot_hip gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_csr_scratch_elems gsn_csr_build_hip "
        "gsn_propagate_self_fwd_hip gsn_fold_weights_fwd_hip gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_fold_weights_bwd_hip gsn_propagate_pad_bwd_hip gsn_bn_act_bwd_from_h_hip gsn_wgrad_hip",
    ],
    "train_gin": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_pad_bwd_hip gsn_propagate_self_bwd_hip",
    ],
    "train_ogb": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_linear_fwd_hip gsn_bn_finalize_act_hip gsn_linear_fwd_hip",
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_pad_bwd_hip gsn_propagate_self_bwd_hip",
    ],
    "eval_grad_general": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_layer_fused_prepared_bytes "
        "gsn_layer_fused_prepared_bytes gsn_layer_fused_prepare_hip gsn_layer_fused_workspace_bytes gsn_layer_fused_fwd_ws_hip",
        "gsn_linear_fwd_hip gsn_bn_act_hip gsn_propagate_self_fwd_hip gsn_fold_weights_fwd_hip gsn_linear_fwd_hip gsn_bn_act_hip gsn_linear_fwd_hip "
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_fold_weights_bwd_hip gsn_propagate_pad_bwd_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_segment_sum_rows_hip",
    ],
    "eval_grad_global": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_layer_fused_supported gsn_mlp_chain_supported "
        "gsn_mlp_chain_supported gsn_segsum_prepare_hip gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
        "gsn_linear_fwd_hip gsn_bn_act_hip gsn_propagate_self_fwd_hip gsn_fold_weights_fwd_hip gsn_linear_fwd_hip gsn_bn_act_hip gsn_linear_fwd_hip "
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_fold_weights_bwd_hip gsn_propagate_pad_bwd_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_segment_sum_rows_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_segment_sum_rows_hip",
    ],
    "eval_grad_gin": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
        "gsn_propagate_self_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip gsn_linear_fwd_hip gsn_bn_act_hip gsn_linear_fwd_hip "
        "gsn_bn_act_bwd_hip gsn_linear_splitk_plan gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_bn_act_bwd_from_h_hip gsn_linear_splitk_plan "
        "gsn_linear_fwd_strided_hip gsn_wgrad_hip gsn_csr_scratch_elems gsn_csr_build_hip gsn_propagate_pad_bwd_hip gsn_propagate_self_bwd_hip",
    ],
    "twin_general": [
        "gsn_csr_scratch_elems gsn_csr_build_hip gsn_linear_fwd_hip gsn_linear_fwd_hip gsn_mlp_chain_supported gsn_mlp_chain_supported "
        "gsn_mlp_chain_fwd_hip gsn_bn_finalize_count_hip gsn_mlp_chain_supported gsn_segsum_prepare_hip gsn_mlp_chain_fwd_hip gsn_mlp_chain_supported "
        "gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip gsn_bn_finalize_count_hip gsn_mlp_chain_supported gsn_mlp_chain_fwd_hip",
        "gsn_propagate_self_fwd_hip gsn_propagate_pad_bwd_hip",
    ],
}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_route_makes_the_recorded_foreign_calls(case):
    phases, outs = run_case(case)
    got = [" ".join(p) for p in phases]
    print(case["name"], got)
    assert got == EXPECTED[case["name"]]
    assert all(bool(torch.isfinite(t).all()) for t in outs)


def test_table_covers_every_rung():
    """The recorded table itself: between them the cases take every route (named by an entry point only that route calls there), and a recorded
    second forward is exactly one foreign call -- the layer kernel."""
    first = {name: phases[0].split() for name, phases in EXPECTED.items()}
    for name, kernel in (("codes_pack", "gsn_layer_fused_fwd_pack16_hip"), ("fused_tagged", "gsn_layer_fused_fwd_pack16_hip"),
                         ("wide_graphs", "gsn_layer_fused_fwd_graphs_hip")):
        assert EXPECTED[name][1] == kernel, name
    for name, entry in (("codes_pack", "gsn_one_hot_pack16_hip"), ("codes_gather_wide", "gsn_code_stage_fwd_hip"),
                        ("fused_rows", "gsn_layer_fused_fwd_ws_hip"), ("wide_graphs", "gsn_layer_fused_fwd_graphs_hip"),
                        ("split_edge", "gsn_edge_split_sum_hip"), ("chain_segsum", "gsn_segsum_prepare_hip"),
                        ("materialised", "gsn_propagate_self_fwd_hip"), ("edgeless", "gsn_propagate_self_fwd_hip"),
                        ("single_linear_msg", "gsn_propagate_self_fwd_hip"), ("gin_local", "gsn_propagate_self_fwd_hip"),
                        ("ogb_mpnn", "gsn_propagate_self_fwd_hip"), ("train_general", "gsn_fold_weights_fwd_hip")):
        assert entry in first[name], (name, entry)
    assert set(EXPECTED) == {c["name"] for c in CASES}
