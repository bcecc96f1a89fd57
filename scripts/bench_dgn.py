#!/usr/bin/env python3
"""Directional GSN timings on one GPU: the native aggregation (csrc/dgn.hip) forward and backward, the DGN layer's train step and the
DGNNet train step (eager and replayed as a HIP graph), each beside the same computation written in composed PyTorch (scatter_reduce
amax / amin, index_add) on the same GPU.  Molecule-shaped batches (synth.zinc_shape_batch) at B = 128 and 4 096 graphs, the HIV config
(d = 70; mean max min dir1-dx dir1-av; identity).  Device-event timing over windows of >= 1 s after a warm-up.

    python scripts/bench_dgn.py [--graphs 128,4096] [--window 1.0] [--only-step]

Prints one JSON line per measurement: time per call, the algorithmic bytes, their share of 8 TB/s, and the gathered bytes E * d * 4
(reads of h[src] that should mostly hit L2 / MALL) apart."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gsn_amd import dgn, graphs, layers, synth  # noqa: E402

AGGS = "mean max min dir1-dx dir1-av"
HBM = 8.0e12


def timed(fn, window):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    one = max(e0.elapsed_time(e1) / 1e3, 1e-6)
    reps = max(5, int(window / one))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def composed(h, ei, ef):
    """The aggregation of the HIV config in composed PyTorch (what a user writes without the kernel)."""
    N, d = h.shape
    src, dst = ei[0], ei[1]
    D = torch.bincount(dst, minlength=N).to(h.dtype).unsqueeze(1)
    has = D > 0
    hs = h[src]
    seg = lambda x: torch.zeros(N, x.shape[1], dtype=h.dtype, device=h.device).index_add(0, dst, x)
    idx = dst.unsqueeze(1).expand(-1, d)
    mean = seg(hs) / D.clamp(min=1)
    mx = torch.zeros(N, d, device=h.device).scatter_reduce(0, idx, hs, "amax", include_self=False)
    mn = torch.zeros(N, d, device=h.device).scatter_reduce(0, idx, hs, "amin", include_self=False)
    w = ef[:, 1:2]
    sabs = seg(w.abs())[dst] + 1e-8
    wdx = w / sabs
    dx = (seg(hs * wdx) - seg(wdx) * h).abs()
    av = seg(hs * (w.abs() / sabs))
    return torch.where(has, torch.cat([mean, mx, mn, dx, av], 1), torch.zeros(1, 5 * d, device=h.device))


def batch(G, seed=0):
    b = synth.zinc_shape_batch(G, seed=seed)
    u, v = b.edge_index
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    ef = np.stack([(lo * 7 + hi * 13 + k) % (3 + k) for k in range(2)], 1).astype(np.float32) - 1.0
    rng = np.random.default_rng(seed)
    codes = np.stack([rng.integers(0, min(dim, 5), size=b.num_nodes) for dim in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1)
    return b, ef, codes


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make_net(dropout_impl=None, dropout=0.3, in_feat_dropout=0.0):
    """The DGNNet of the HIV config (4 layers, d = 70); ``dropout_impl``: "torch", "native" (gsn_amd.dropout) or None (GSN_DROPOUT)."""
    return dgn.DGNNet(dict(L=4, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean",
                           in_feat_dropout=in_feat_dropout, dropout=dropout, graph_norm=False, batch_norm=True, aggregators=AGGS, scalers="identity",
                           towers=5, divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1, posttrans_layers=1,
                           pos_enc_dim=0, avg_d={"log": 1.0}, device="cuda", dropout_impl=dropout_impl)).cuda().train()


def bench(G, window, only_step, optimizer="adam", dropout_impl=None):
    b, ef_np, codes_np = batch(G)
    g = dgn.DGNGraph.from_batch(b, edge_field=ef_np)
    N, E, d, A = b.num_nodes, b.num_edges, 70, 5
    ei, ef = g.edge_index, g.edata["eig"]
    torch.manual_seed(0)
    h = torch.randn(N, d, device="cuda", requires_grad=True)
    common = dict(graphs=G, nodes=N, edges=E, d=d)
    csr = 4 * (2 * (N + 1) + 4 * E)                            # two seg_ptr, perm + src (target CSR), perm (source CSR), int32
    field = 4 * E * 1                                          # the one column the dir kinds read
    fwd_bytes = 4 * N * d + 4 * N * A * d + csr // 2 + field
    bwd_bytes = (4 * N * d + 4 * N * A * d + csr // 2 + field + 4 * E * d      # pass 1: h_in, grad_out, CSR, field; grad_msg written
                 + 4 * E * d + 4 * N * d * 2 + 4 * (N + 1 + E))              # pass 2: grad_msg read, grad_h read + written, source CSR
    gathered = 4 * E * d
    if not only_step:
        spec = dgn._make_spec(AGGS, "identity", None)
        f = lambda: dgn.dgn_aggregate(h.detach(), ei, None, edge_field=ef, spec=spec)
        t = timed(f, window)
        emit(what="aggregate_fwd", native=True, us=t * 1e6, bytes=fwd_bytes, hbm_frac=fwd_bytes / t / HBM, gathered_bytes=gathered, **common)
        y = dgn.dgn_aggregate(h, ei, None, edge_field=ef, spec=spec)
        gy = torch.randn_like(y)
        fb = lambda: torch.autograd.grad(y, [h], gy, retain_graph=True)
        t = timed(fb, window)
        emit(what="aggregate_bwd", native=True, us=t * 1e6, bytes=bwd_bytes, hbm_frac=bwd_bytes / t / HBM, gathered_bytes=2 * gathered, **common)
        tc = timed(lambda: composed(h.detach(), ei, ef), window)
        emit(what="aggregate_fwd", native=False, us=tc * 1e6, **common)
        yc = composed(h, ei, ef)
        tcb = timed(lambda: torch.autograd.grad(yc, [h], gy, retain_graph=True), window)
        emit(what="aggregate_bwd", native=False, us=tcb * 1e6, **common)
        # the layer's train step (forward + backward of DGNLayerSimple, BatchNorm on batch statistics)
        layer = dgn.DGNLayerSimple(d, d, 0.0, False, True, AGGS.split(), ["identity"], True, None).cuda().train()
        w = torch.randn(N, d, device="cuda")

        def layer_step():
            y = layer(g, h, None, g.snorm_n)
            torch.autograd.grad((y * w).sum(), [h] + list(layer.parameters()))
        t = timed(layer_step, window)
        emit(what="layer_train_step", native=True, us=t * 1e6, **common)

        def layer_step_composed():
            a = composed(h, ei, ef)
            y = torch.nn.functional.linear(a, layer.posttrans.fully_connected[0].linear.weight, layer.posttrans.fully_connected[0].linear.bias)
            y = h + torch.relu(torch.nn.functional.batch_norm(y, None, None, layer.batchnorm_h.weight, layer.batchnorm_h.bias, True))
            torch.autograd.grad((y * w).sum(), [h] + list(layer.parameters()))
        t = timed(layer_step_composed, window)
        emit(what="layer_train_step", native=False, us=t * 1e6, **common)
    # the DGNNet train step: forward, BCE loss, backward, Adam
    net = make_net(dropout_impl)
    if optimizer == "adam_native":
        from gsn_amd import optim
        opt = optim.Adam(net.parameters(), lr=0.01, weight_decay=3e-6)
    else:
        opt = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=3e-6, capturable=True)
    common = dict(common, optimizer=optimizer, dropout=net.dropout_impl)
    codes = torch.from_numpy(codes_np).cuda()
    labels = torch.from_numpy((np.arange(G) % 2).astype(np.float32)).cuda()

    def loss_fn():
        return net.loss(net(g, codes, None, g.snorm_n, None), labels)

    def eager():
        opt.zero_grad(set_to_none=False)
        loss_fn().backward()
        opt.step()
    t = timed(eager, window)
    emit(what="net_train_step", native=True, graph=False, us=t * 1e6, **common)
    gstep = graphs.GraphedTrainStep(loss_fn, opt, allreduce=False)
    t = timed(gstep, window)
    emit(what="net_train_step", native=True, graph=True, us=t * 1e6, **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="128,4096")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "adam_native"], help="adam_native: gsn_amd.optim.Adam, one HIP launch per step")
    ap.add_argument("--dropout", default=None, choices=["torch", "native"],
                    help="native: gsn_amd.dropout in the net's layers, one HIP launch per call (default: GSN_DROPOUT, else torch)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dgn.py measures on the GPU; there is no CPU fallback"
    for G in [int(x) for x in a.graphs.split(",")]:
        bench(G, a.window, a.only_step, a.optimizer, a.dropout)
        layers.drop_input_caches()


if __name__ == "__main__":
    main()
