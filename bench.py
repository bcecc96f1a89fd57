#!/usr/bin/env python3
"""Benchmark of the hot path named by BASELINE.json: orbit counting + GSN-e forward on ZINC-shaped batches.

One "step" = one pass over one batch of G synthetic ZINC-shaped graphs resident in HBM:
    (1) gsn_count_encode_hip    cycle_graph k = 3..6, id_scope=local (GSN-e), non-induced; the counts [E, 4] leave the kernel
                                 as the per-column one-hot of min(count, 2) -> float [E, 12] (the reference: int64 identifiers,
                                 then DiscreteEmbedding('one_hot_encoder'), utils_graph_learning.py:78 / :170-187); after the
                                 timed region the int64 counts of the same batch are produced by gsn_count_hip and checked
    (2) GSN_edge_sparse forward  layer 0 of BASELINE config 2: msg_kind=general, d_in=28, d_ef=4, d_id=12, d_h=d_msg=d_up=128,
                                 bn=True, eval mode; includes building the target-sorted CSR (cache cleared every step)
Prints ONE JSON line (rank 0).  Multi-GPU: one process per GPU (torch.distributed / RCCL only for the barrier and the
max-over-ranks timing); graphs are sharded across ranks, the data path has no collective ("weak" scaling: G per GPU fixed).

A plain run sets up, warms up, times the K steps and prints the headline line (`value`, `ms_per_step`, ...).  `--full` adds what the
headline does not need: the timed batch against the oracle, per-kernel times and the roofline, HIP-graph replays, the step variants,
other sizes and configurations, the RCCL all-reduce and the CPU baseline (`--no-extras` / `--no-graph` / `--no-cpu-baseline` trim those).
`--dump-outputs DIR` writes what the last timed step computed (a fixed seeded sample of its rows, dump_outputs) as DIR/<name>.npy.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--graphs G] [--full] [--dump-outputs DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PACK_ONLY_IDS = os.environ.get("GSN_BENCH_PACK_ONLY_IDS", "1") != "0"      # headline: no fp32 one-hot identifier rows (0: written, as rounds 2-4 / early r05)
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: fp32 MFMA (v_mfma_f32_32x32x2_f32) dense peak
MFMA_BF16_PEAK_TF = 2500.0  # MI355X_MICROARCH.md: bf16 MFMA (v_mfma_f32_32x32x16_bf16) dense peak (no sparsity)
BF16X6 = os.environ.get("GSN_CHAIN_BF16X6", "64") != "0"   # chain kernels: 6 bf16 plane products per fp32 product (default)


def make_batch(n_graphs, seed):
    """n_graphs distinct seeded ZINC-shaped graphs (generation is Python-side and not timed: ~0.16 ms per graph)."""
    from gsn_amd import synth
    return synth.zinc_shape_batch(n_graphs, seed=seed)


CTOR = dict(d_in=28, d_ef=4, d_id=12, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128,
            d_up=128, d_h=[128], seed=0, activation_name="relu", bn=True, msg_kind="general", flow="source_to_target")


def cpu_baseline(seed):
    """The oracle (CPU port of the reference path: oracle/count_oracle.c + plain PyTorch fp32 layer) timed on this box's host
    cores on bounded samples of the same workload: at 1 thread (the reference's default --num_threads 1, main.py:519-520),
    at all host cores, and at 32 threads (where this port peaks: the PyTorch CPU layer slows down beyond that on batches of
    small graphs).  `value` / `cores` are the all-cores run; the other two ride along."""
    import torch
    import networkx as nx
    from gsn_amd import flags, synth, layers
    from oracle import oracle
    pats = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
    torch.manual_seed(0)
    layer = layers.GSN_edge_sparse(**CTOR).eval()
    sd = {k: v.clone() for k, v in layer.state_dict().items()}

    def run(n_graphs, threads, budget_s):
        b = synth.zinc_shape_batch(n_graphs, seed=seed)
        local = b.edge_index - np.repeat(b.node_ptr[:-1], np.diff(b.edge_ptr))[None, :]
        x = torch.nn.functional.one_hot(torch.from_numpy(b.atom_type), 28).float()
        ef = torch.nn.functional.one_hot(torch.from_numpy(b.bond_type), 4).float()
        ei = torch.from_numpy(b.edge_index)
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        reps = 0
        while True:
            ids = oracle.counts2ids("edge", False, b.node_ptr, b.edge_ptr, local, pats, n_threads=threads)
            idt = torch.from_numpy(ids).clamp(max=2)
            idf = torch.nn.functional.one_hot(idt, 3).reshape(idt.shape[0], 12).float()
            with torch.no_grad():
                oracle.layer_forward("GSN_edge_sparse", CTOR, sd, x, ei, identifiers=idf, degrees=None, edge_features=ef)
            reps += 1
            dt = time.perf_counter() - t0
            if dt > budget_s:
                break
        return {"value": round(reps * n_graphs / dt, 1), "unit": "graphs/s", "cores": threads,
                "sample": "%d passes over %d ZINC-shaped graphs, %d thread%s, %.1f s" % (reps, n_graphs, threads, "" if threads == 1 else "s", dt)}
    ncpu = os.cpu_count() or 1
    one = run(1024, 1, 5.0)
    allc = run(8192, ncpu, 6.0) if ncpu > 1 else one
    mid = run(8192, 32, 6.0) if ncpu > 32 else None
    # `value` / `cores`: the configuration this port is fastest at (it is a baseline, not a target); the reference's default
    # (1 thread) and the all-cores run are reported beside it.  On the 256-thread GPU host the all-cores run is the SLOWEST
    # (OpenMP over 8192 small graphs + 256 PyTorch threads on matrices of a few thousand rows: oversubscription).
    cands = [c for c in (one, allc, mid) if c is not None]
    best = max(cands, key=lambda c: c["value"])
    return dict(best, kind="port", host_cpu_count=ncpu, one_thread=one, all_cores=allc,
                what="oracle/count_oracle.c (OpenMP over graphs) + plain PyTorch fp32 layer forward; value/cores = the fastest of "
                     "1 thread / 32 threads / all host cores")


def verify_tile(plan, b, ids_out, y, layer, n_check):
    """After the timed region: the counts and the layer output of the first `n_check` graphs of the timed batch against the
    oracle (the timed step itself never checks)."""
    import torch
    import networkx as nx
    from oracle import oracle
    g = min(n_check, b.num_graphs)
    n1, e1 = int(b.node_ptr[g]), int(b.edge_ptr[g])
    pats = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
    local = b.edge_index[:, :e1] - np.repeat(b.node_ptr[:g], np.diff(b.edge_ptr[:g + 1]))[None, :]
    ref = oracle.counts2ids("edge", False, b.node_ptr[:g + 1], b.edge_ptr[:g + 1], local, pats, n_threads=min(os.cpu_count() or 1, 32))
    got = ids_out[:e1].cpu().numpy()
    counts_ok = bool(np.array_equal(got, ref))
    sd = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}
    x = torch.nn.functional.one_hot(torch.from_numpy(b.atom_type[:n1]), 28).float()
    ef = torch.nn.functional.one_hot(torch.from_numpy(b.bond_type[:e1]), 4).float()
    idf = torch.nn.functional.one_hot(torch.from_numpy(ref).clamp(max=2), 3).reshape(e1, 12).float()
    with torch.no_grad():
        yref = oracle.layer_forward("GSN_edge_sparse", CTOR, sd, x, torch.from_numpy(b.edge_index[:, :e1]), identifiers=idf, degrees=None, edge_features=ef)
    ygot = y[:n1].cpu()
    err_max = float((ygot - yref).abs().max() / yref.abs().max())
    # element-wise: |got - ref| <= 1e-5 |ref| + 1e-5 * (row scale): the floor is 1e-5 of the row's largest |value|
    floor = 1e-5 * yref.abs().amax(dim=1, keepdim=True)
    diff = (ygot - yref).abs()
    elem_ok = bool((diff <= 1e-5 * yref.abs() + floor).all())
    # how much the floor is needed: elements that fail the PURE relative test |got - ref| <= 1e-5 |ref|, and how small they
    # are against their row (cancellation-small elements: their absolute error is that of the row's large ones)
    # fp64 referee: the same layer in float64 (the oracle's code on .double() inputs); PURE relative errors, no floor,
    # of (i) the HIP kernel and (ii) the fp32 oracle against it -- element-wise, over the elements above 1e-3 of their row's largest magnitude
    # (below that a 1e-5 relative bar asks for more digits than fp32 sums of 128-260 terms carry on either side)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        y64 = oracle.layer_forward("GSN_edge_sparse", CTOR, sd64, x.double(), torch.from_numpy(b.edge_index[:, :e1]), identifiers=idf.double(), degrees=None,
                                   edge_features=ef.double())
    rowmax64 = y64.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)
    big = y64.abs() >= 1e-3 * rowmax64
    rel_hip = ((ygot.double() - y64).abs() / y64.abs().clamp_min(1e-300))
    rel_orc = ((yref.double() - y64).abs() / y64.abs().clamp_min(1e-300))
    worse = big & (rel_hip > 2.0 * rel_orc) & (rel_hip > 1e-6)      # elements where the HIP kernel is more than 2x further from fp64 than the fp32 oracle
    fp64 = {"elements_above_1e-3_of_rowmax": int(big.sum()),
            "hip_max_rel_err_vs_fp64": float("%.3g" % float(rel_hip[big].max())), "oracle_fp32_max_rel_err_vs_fp64": float("%.3g" % float(rel_orc[big].max())),
            "hip_mean_rel_err_vs_fp64": float("%.3g" % float(rel_hip[big].mean())), "oracle_fp32_mean_rel_err_vs_fp64": float("%.3g" % float(rel_orc[big].mean())),
            "hip_elements_over_1e-5_rel": int((big & (rel_hip > 1e-5)).sum()), "oracle_fp32_elements_over_1e-5_rel": int((big & (rel_orc > 1e-5)).sum()),
            "hip_max_err_over_rowmax_vs_fp64": float("%.3g" % float(((ygot.double() - y64).abs() / rowmax64).max())),
            "oracle_fp32_max_err_over_rowmax_vs_fp64": float("%.3g" % float(((yref.double() - y64).abs() / rowmax64).max())),
            "elements_hip_over_2x_the_oracle_error": int(worse.sum()),
            # per element against the fp32 oracle's own worst error IN THE SAME ROW (two fp32 evaluations of one row differ element by element; what
            # bounds both is the row's scale): elements where the HIP kernel's error exceeds twice that
            "elements_hip_error_over_2x_the_oracle_worst_error_of_the_row": int(((ygot.double() - y64).abs() > 2.0 * (yref.double() - y64).abs().amax(dim=1, keepdim=True)).sum()),
            "largest_abs_ref_over_rowmax_among_those": float("%.3g" % (float((y64.abs() / rowmax64)[worse].max()) if int(worse.sum()) else 0.0)),
            "hip_max_rel_err_vs_fp64_within_2x_of_the_fp32_oracle": bool(float(rel_hip[big].max()) <= 2.0 * max(float(rel_orc[big].max()), 1e-7)),
            "note": "pure relative errors |v - v64| / |v64| over the elements with |v64| >= 1e-3 of their row's largest magnitude; v64 = the oracle's layer in float64"}
    pure_bad = diff > 1e-5 * yref.abs()
    n_bad = int(pure_bad.sum())
    rel_to_row = (yref.abs() / yref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30))[pure_bad]
    return {"graphs": g, "counts_bit_exact": counts_ok, "layer_max_err_over_max": float("%.3g" % err_max),
            "layer_elementwise_1e-5_rel_plus_1e-5_rowmax": elem_ok,
            "layer_elements": int(yref.numel()), "layer_elements_failing_pure_1e-5_relative": n_bad,
            "layer_fraction_failing_pure_1e-5_relative": float("%.3g" % (n_bad / max(int(yref.numel()), 1))),
            "largest_abs_ref_over_rowmax_among_those": float("%.3g" % (float(rel_to_row.max()) if n_bad else 0.0)),
            "largest_abs_err_over_rowmax_among_those": float("%.3g" % (float((diff / yref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30))[pure_bad].max()) if n_bad else 0.0)),
            "fp64_referee": fp64}


def work_figures(plan_patterns, ids_out):
    """SURVEY 8(d) counting work figures derivable from the output alone: occurrences x positions = sum of all counts;
    maps = sum_p aut_p * (sum of pattern p's columns) / (2 |E(H_p)|)  (edge mode)."""
    from gsn_amd import patterns
    col_sums = ids_out.sum(dim=0).cpu().numpy().astype(np.float64)
    maps, c0 = 0.0, 0
    for el in plan_patterns:
        info = patterns.analyse(el, False)
        w = info["n_edge_orbits"]
        maps += info["aut_count"] * col_sums[c0:c0 + w].sum() / float(len(info["arcs"]))
        c0 += w
    return float(col_sums.sum()), float(maps)


def full_model_closure(dev, gm, batch=None, check=True):
    """count + the FULL model of BASELINE configs[1] (GNNSubstructures, 4 layers: layer 0 is GSN_edge_sparse, layers 1-3
    MPNN_edge_sparse with K = 260 edge rows -- the any-shape dense kernels; one-hot encoders, jk, sum readout, eval) over `gm`
    ZINC-shaped graphs -> (step function, gm).  Also used by scripts/profile_full_model.py."""
    import types
    import networkx as nx
    import torch
    from gsn_amd import flags, layers, models
    from gsn_amd.counting import CountPlan, count_batch
    if batch is None:
        b = make_batch(gm, seed=1000)
        node_ptr = torch.from_numpy(b.node_ptr).to(dev)
        edge_ptr = torch.from_numpy(b.edge_ptr).to(dev)
        ei = torch.from_numpy(b.edge_index).to(dev)
        plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
        max_nodes, max_edges = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    else:
        b, node_ptr, edge_ptr, ei, plan, max_nodes, max_edges = batch
    L4, d4 = 4, 128
    kw = dict(seed=0, model_name="GSN_edge_sparse", readout="sum", dropout_features=[0.0] * (L4 + 1), bn=[True] * L4,
              final_projection=[False] * L4 + [True], inject_ids=False, inject_edge_features=True, random_features=False,
              id_scope="local", d_msg=[d4] * L4, d_out=[d4] * L4, d_h=[[d4]] * L4, aggr="add", flow="source_to_target",
              msg_kind="general", train_eps=[False] * L4, activation_mlp="relu", bn_mlp=True, jk_mlp=True, degree_embedding="None",
              degree_as_tag=[False] * L4, retain_features=[True] * L4, multi_embedding_aggr="sum", input_node_encoder="one_hot_encoder",
              d_out_node_encoder=d4, edge_encoder="one_hot_encoder", d_out_edge_encoder=[d4] * L4, id_embedding="one_hot_encoder",
              d_out_id_embedding=d4, d_out_degree_embedding=d4, extend_dims=True, activation="relu")
    torch.manual_seed(0)
    n4, e4 = int(b.node_ptr[gm]), int(b.edge_ptr[gm])
    model = models.GNNSubstructures(1, 1, None, [3, 3, 3, 3], 1, [28], [4], None, None, **kw).to(dev).eval()
    np4, ep4 = node_ptr[:gm + 1].contiguous(), edge_ptr[:gm + 1].contiguous()
    ei4 = ei[:, :e4].contiguous()
    ids4 = torch.empty((e4, plan.n_cols), dtype=torch.int64, device=dev)
    data4 = types.SimpleNamespace(x=torch.from_numpy(b.atom_type[:n4]).unsqueeze(1).to(dev), edge_index=ei4,
                                  edge_features=torch.from_numpy(b.bond_type[:e4]).unsqueeze(1).to(dev), identifiers=None,
                                  batch=torch.from_numpy(np.asarray(b.batch)[:n4].astype(np.int64)).to(dev), degrees=torch.zeros(n4, device=dev),
                                  graph_partition=(np4, ep4, max_nodes, max_edges, check))

    def step_model():
        layers._CSR_CACHE.clear()
        count_batch(plan, np4, ep4, ei4, ids_are_global=True, max_nodes=max_nodes, max_edges=max_edges, device=dev, out=ids4, check=False)
        data4.identifiers = ids4.clamp(max=2)
        with torch.no_grad():
            return model(data4)
    return step_model, gm


def dry_run(args):
    """--dry-run: everything around the kernels (rank launch, process group, barrier-bracketed timing, MAX over ranks, one
    JSON line from rank 0) with an empty step, so the N > 1 entry point is testable on a box without GPUs (gloo)."""
    import torch
    from gsn_amd import dist as gdist
    rank, world, _, dist = gdist.init_from_env(args.backend, None)
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks" % (args.gpus, world))

    def sync():
        if dist is not None:
            dist.barrier()
    for _ in range(args.warmup):
        pass
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001 * (1 + rank))          # ranks differ: the reported time must be the slowest rank's
    sync()
    dt = gdist.max_over_ranks(time.perf_counter() - t0)
    if rank == 0:
        print(json.dumps({"metric": "graphs/sec (orbit-count + GSN-e fwd), ZINC-shape batch; % HBM roofline", "value": None,
                          "unit": "graphs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dry_run": True, "backend": args.backend,
                          "config": {"workload": "none (plumbing check: empty step)", "parallelism": "graph-shard x%d" % world}}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def spin_up(fn, min_ms=60.0):
    """Untimed calls of ``fn`` until ~min_ms of device work are behind us: every supplementary figure is taken right behind load, not behind the
    host-side set-up in front of it (the device drops its clocks while it idles)."""
    import torch
    t0 = time.perf_counter()
    while True:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        if (time.perf_counter() - t0) * 1e3 >= min_ms:
            return


def rr_tiling(seg, n_nodes, grid=256, unit=32):
    """The tiles and 32-row edge blocks csrc/layer_rr.hip walks for this CSR (its iterator restated): 2048 node ranges, tiles of <= 32
    nodes whose in-edges are a whole number of 64-row chunks where the degrees allow it, blocks of <= 32 edge rows.  For the roofline's
    executed-MFMA count (outside the timed region)."""
    n_tiles_nominal = (n_nodes + 31) // 32
    n_ranges = min(grid * 8, n_tiles_nominal)            # (layer_w.hip: 256 workgroups x 4 waves = the same 1024 with grid = 128)
    tiles = blocks = 0
    for r in range(n_ranges):
        m, end = n_nodes * r // n_ranges, n_nodes * (r + 1) // n_ranges
        while m < end:
            nmax = min(32, end - m)
            cnt = seg[m:m + nmax + 1] - seg[m]
            nn = nmax
            if cnt[nmax] > 64:
                cap = int(cnt[nmax]) // 64 * 64
                nn = max(1, int(np.searchsorted(cnt, cap, side="right")) - 1)
            tiles += 1
            blocks += (int(cnt[nn]) + unit - 1) // unit
            m += nn
    return tiles, blocks


def small_batch_steps(plan, layer, dev, graphs=True):
    """the reference's real batch sizes (32 / 128 graphs per step).  Wall time of count + encode + CSR + layer-0 forward
    per step: eager (host-bound: ~8 launches) and replayed from one captured HIP graph (what is left is the serial latency of the
    small dependent kernels).  Supplementary, never `value`."""
    import torch
    from gsn_amd import flags, layers
    from gsn_amd.counting import count_batch
    out = {}
    for G in (32, 128):
        b = make_batch(G, seed=G)
        N, E = b.num_nodes, b.num_edges
        mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
        node_ptr, edge_ptr = torch.from_numpy(b.node_ptr).to(dev), torch.from_numpy(b.edge_ptr).to(dev)
        ei = torch.from_numpy(b.edge_index).to(dev)
        x = torch.nn.functional.one_hot(torch.from_numpy(b.atom_type), 28).float().to(dev)
        ef = torch.nn.functional.one_hot(torch.from_numpy(b.bond_type), 4).float().to(dev)
        deg = torch.zeros(N, device=dev)
        idf = torch.empty((E, 12), dtype=torch.float32, device=dev)
        layers.set_graph_partition(ei, node_ptr, edge_ptr, mn, me, check=False)

        def step():
            layers._CSR_CACHE.clear()
            count_batch(plan, node_ptr, edge_ptr, ei, ids_are_global=True, max_nodes=mn, max_edges=me, device=dev, check=False,
                        encode=([3, 3, 3, 3], True), counts=False, encoded_out=idf)
            with torch.no_grad():
                return layer(x, ei, identifiers=idf, degrees=deg, edge_features=ef)
        for _ in range(30):
            step()
        torch.cuda.synchronize()
        reps = 300
        t0 = time.perf_counter()
        for _ in range(reps):
            y_ref = step()
        torch.cuda.synchronize()
        rec = {"graphs": G, "eager_us": round((time.perf_counter() - t0) / reps * 1e6, 1)}
        # the same work as ONE host call (gsn_amd.step.CountLayerStep: integer codes in, int64 identifiers + layer rows out; the headline's form)
        try:
            from gsn_amd.step import CountLayerStep
            stp = CountLayerStep(plan, layer, [3, 3, 3, 3], clamp=True)
            xc_s = layers.Codes(torch.from_numpy(b.atom_type).to(dev), [28])
            efc_s = layers.Codes(torch.from_numpy(b.bond_type).to(dev), [4])
            one = lambda: stp(node_ptr, edge_ptr, ei, xc_s, efc_s, mn, me)[1]
            for _ in range(30):
                one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                y_one = one()
            torch.cuda.synchronize()
            rec["one_call_eager_us"] = round((time.perf_counter() - t0) / reps * 1e6, 1)
            # (the composed step above runs the layer on dense fp32 one-hot rows -- csrc/layer_rr.hip --, the one-call step on exact fp16 packs --
            #  csrc/layer_rp.hip: the same products in another order of accumulation)
            rec["one_call_max_diff_over_max_vs_eager"] = float("%.3g" % (float((y_one - y_ref).abs().max()) / float(y_ref.abs().max())))
        except Exception as e:
            rec["one_call_error"] = str(e)[:160]
        if not graphs:                 # (--no-graph: stream capture cannot free memory without the caching allocator, scripts/oob_check.sh)
            out["B%d" % G] = rec
            continue
        try:
            from gsn_amd.graphs import GraphedStep
            g = GraphedStep(step, warmup=3, device=dev)          # (the product's capture helper: side-stream warm-up, capture, replay)
            for _ in range(30):
                g()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                y_static = g()
            torch.cuda.synchronize()
            rec["hip_graph_us"] = round((time.perf_counter() - t0) / reps * 1e6, 1)
            rec["hip_graph_matches_eager"] = bool(torch.equal(y_static, y_ref))
        except Exception as e:       # capture is best effort
            rec["hip_graph_error"] = str(e)[:160]
        out["B%d" % G] = rec
    # the whole model of BASELINE configs[1] (count + 4 layers + encoders + readout) at the reference's batch size, eager and replayed
    try:
        from gsn_amd.graphs import GraphedStep
        mstep, _ = full_model_closure(dev, 128, check=False)
        for _ in range(10):
            y_ref = mstep()
        torch.cuda.synchronize()
        reps = 100
        t0 = time.perf_counter()
        for _ in range(reps):
            y_ref = mstep()
        torch.cuda.synchronize()
        rec = {"graphs": 128, "eager_us": round((time.perf_counter() - t0) / reps * 1e6, 1)}
        if not graphs:
            out["full_model_B128"] = rec
            return out
        g = GraphedStep(mstep, warmup=2, device=dev)
        for _ in range(10):
            g()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            y_static = g()
        torch.cuda.synchronize()
        rec["hip_graph_us"] = round((time.perf_counter() - t0) / reps * 1e6, 1)
        rec["hip_graph_matches_eager"] = bool(torch.equal(y_static, y_ref))
        out["full_model_B128"] = rec
    except Exception as e:
        out["full_model_B128"] = {"error": str(e)[:160]}
    return out


def propagate_figures(b, dev):
    """the stand-alone per-target sum (gsn_propagate_fwd_hip, the aggregation of the gin / ogb layers and the fallback
    of the others) on the bench batch as a fraction of the HBM peak -- the two cases of scripts/bench_propagate.py that the 0.70 target
    is quoted on: the scatter-add of per-edge messages with d = 128 and the ogb message relu(x_j + id_e + e) with d = 300.
    Algorithmic bytes: the CSR's three int32 arrays + seg_ptr, every message operand once, the output once."""
    import torch
    from gsn_amd import flags, layers
    N, E = b.num_nodes, b.num_edges
    ei = torch.from_numpy(b.edge_index).to(dev)
    out = {}
    for name, kind, da, db, dc in (("scatter_add_messages_d128", 0, 0, 128, 0), ("ogb_relu_sum_d300", 1, 300, 300, 300)):
        a = torch.randn(N, da, device=dev) if da else None
        bb = torch.randn(E, db, device=dev) if db else None
        c = torch.randn(E, dc, device=dev) if dc else None
        with torch.no_grad():
            y = layers.propagate(kind, ei, 1, N, a=a, b=bb, c=c)
            spin_up(lambda: layers.propagate(kind, ei, 1, N, a=a, b=bb, c=c))
            flags.KERNEL_TIMER = {}
            for _ in range(10):
                layers.propagate(kind, ei, 1, N, a=a, b=bb, c=c)
            torch.cuda.synchronize()
        evs = flags.KERNEL_TIMER.get("propagate_fwd", [])
        flags.KERNEL_TIMER = None
        ms = sum(e0.elapsed_time(e1) for e0, e1, _ in evs) / max(len(evs), 1)
        byt = 12.0 * E + 4.0 * (N + 1) + 4.0 * (N * da + E * db + E * dc) + 4.0 * N * y.shape[1]
        out[name] = {"ms": round(ms, 4), "GBps": round(byt / ms / 1e6, 1), "hbm_frac": round(byt / ms / 1e6 / HBM_PEAK_GBS, 4)}
        del a, bb, c, y
    return out


def float_input_layer(layer, b, ei, dev):
    """The layer launch alone with real-valued inputs (no row exact in fp16: three plane products in the edge stage, every row scaled,
    the activated rows as three bf16 planes) beside the one-hot headline: the best case is not the only case."""
    import torch
    from gsn_amd import flags, layers
    N, E = b.num_nodes, b.num_edges
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 28, generator=g).to(dev)
    ids = torch.randn(E, 12, generator=g).to(dev)
    ef = torch.randn(E, 4, generator=g).to(dev)
    deg = torch.zeros(N, device=dev)
    with torch.no_grad():
        spin_up(lambda: layer(x, ei, identifiers=ids, degrees=deg, edge_features=ef))
        flags.KERNEL_TIMER = {}
        for _ in range(10):
            layer(x, ei, identifiers=ids, degrees=deg, edge_features=ef)
        torch.cuda.synchronize()
    evs = flags.KERNEL_TIMER.get("layer_fused", [])
    flags.KERNEL_TIMER = None
    ms = sum(e0.elapsed_time(e1) for e0, e1, _ in evs) / max(len(evs), 1)
    return {"layer_launch_ms": round(ms, 4)}


def g_tiling(node_ptr, seg, n_wg=256, rows=128):
    """(workgroup tiles, 32-row wave tiles in use, edge rounds) of csrc/layer_g.hip on this batch: every workgroup takes its share of the
    graphs in runs of whole graphs of <= 128 vertices; a wave's rounds = the largest in-degree among its 32 targets"""
    G = len(node_ptr) - 1
    n_wg = min(n_wg, G)
    deg = np.diff(seg)
    tiles = wave_tiles = rounds = 0
    for w in range(n_wg):
        g, g_end = G * w // n_wg, G * (w + 1) // n_wg
        while g < g_end:
            k = max(1, int(np.searchsorted(node_ptr[g + 1:min(g_end, g + 63) + 1], node_ptr[g] + rows, side="right")))
            n0, n1 = int(node_ptr[g]), int(node_ptr[g + k])
            tiles += 1
            for r in range(n0, n1, 32):
                wave_tiles += 1
                d = deg[r:min(r + 32, n1)]
                rounds += int(d.max()) if len(d) else 0
            g += k
    return tiles, wave_tiles, rounds


def wide_layer(b, ei, dev):
    """A hidden layer of the d = 128 model on the bench batch (GSN_edge_sparse, d_in = 128, K = 272 edge rows), on the collated batch with
    its graph boundaries registered (what gsn_amd.models does): csrc/layer_g.hip -- node products once per node on tiles of whole graphs.
    Executed MFMA flops per launch: per 32-row wave tile 288 (x against [Wj | Wi | W0x]) + 100 (S part of node stage 0 with its bias
    product) + 96 (node stage 1) products of 32 x 32 x 16, + 12 per edge round.  `layer_w`: the same layer on csrc/layer_w.hip (edge
    rows multiplied by all 272 columns; the kernel of a batch without registered boundaries or with a graph above 128 vertices)."""
    import torch
    from gsn_amd import flags, layers
    N, E = b.num_nodes, b.num_edges
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, 128, generator=g).relu().to(dev)
    ids = torch.randn(E, 12, generator=g).abs().to(dev)
    ef = torch.randn(E, 4, generator=g).to(dev)
    deg = torch.zeros(N, device=dev)
    torch.manual_seed(0)
    ctor = dict(d_in=128, d_ef=4, d_id=12, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128, d_up=128,
                d_h=[128], seed=0, activation_name="relu", bn=True, msg_kind="general", flow="source_to_target")
    layer = layers.GSN_edge_sparse(**ctor).to(dev).eval()
    eiw = ei.clone()
    layers.set_graph_partition(eiw, torch.from_numpy(b.node_ptr).to(dev), torch.from_numpy(b.edge_ptr).to(dev),
                               int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max()))
    out = {}
    ys = {}
    for name, flag in (("g", True), ("w", False)):
        was = flags.GRAPH_ALIGNED_LAYER
        flags.GRAPH_ALIGNED_LAYER = flag
        try:
            with torch.no_grad():
                spin_up(lambda: layer(x, eiw, identifiers=ids, degrees=deg, edge_features=ef))
                flags.KERNEL_TIMER = {}
                for _ in range(10):
                    ys[name] = layer(x, eiw, identifiers=ids, degrees=deg, edge_features=ef)
                torch.cuda.synchronize()
            evs = flags.KERNEL_TIMER.get("layer_fused", [])
        finally:
            flags.KERNEL_TIMER = None
            flags.GRAPH_ALIGNED_LAYER = was
        if not evs:
            return {"error": "the layer did not take the one-launch path"}
        out[name] = sum(e0.elapsed_time(e1) for e0, e1, _ in evs) / len(evs)
    ms = out["g"]
    b_alg = 16.0 * E + 4.0 * (N * 128 + E * 16 + N * 128)
    seg = np.concatenate([[0], np.cumsum(np.bincount(b.edge_index[1], minlength=N))])
    tiles, wave_tiles, rounds = g_tiling(np.asarray(b.node_ptr), seg)
    f_exec = 32768.0 * (wave_tiles * 484 + rounds * 12)
    n_t, n_b = rr_tiling(seg, N, grid=128, unit=64)
    f_exec_w = 32768.0 * (n_b * 456 + n_t * 288)
    ref = ys["w"]
    same = bool(((ys["g"] - ref).abs() <= 1e-5 * ref.abs() + 1e-5 * ref.abs().amax(dim=1, keepdim=True)).all())
    return {"ms": round(ms, 4), "kernel": "layer_fused_kernel_g", "algorithmic_bytes": int(b_alg), "hbm_GBs": round(b_alg / ms / 1e6, 1),
            "hbm_frac": round(b_alg / ms / 1e6 / 8000.0, 4), "mfma_executed_TFLOPs": round(f_exec / ms / 1e9, 1),
            "mfma_frac": round(f_exec / ms / 1e9 / 2500.0, 4), "workgroup_tiles": int(tiles), "wave_tiles": int(wave_tiles),
            "row_occupancy": round(N / (32.0 * wave_tiles), 4), "edge_rounds": int(rounds),
            "layer_w": {"ms": round(out["w"], 4), "hbm_frac": round(b_alg / out["w"] / 1e6 / 8000.0, 4),
                        "mfma_executed_TFLOPs": round(f_exec_w / out["w"] / 1e9, 1), "mfma_frac": round(f_exec_w / out["w"] / 1e9 / 2500.0, 4),
                        "note": "row-exponent pass + layer_fused_kernel_w, HIP events around both"},
            "equal_to_layer_w_elementwise_1e-5": same,
            "note": "graph boundaries registered (layers.set_graph_partition); one launch, HIP events around it"}


def train_step_config4(dev):
    """BASELINE configs[3] (ogbg-molhiv GSN-e TRAINING): one optimisation step of the 5 x 300 virtual-node model on 4096 molhiv-shaped
    graphs -- forward, backward (HIP adjoints), gradient bucket, SGD (scripts/train_step_molhiv.py; supplementary, never `value`)."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("train_step_molhiv", os.path.join(os.path.dirname(os.path.abspath(__file__)), "scripts", "train_step_molhiv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.run(types.SimpleNamespace(batch=4096, steps=20, warmup=10, layers=5, d=300), dev)
    out = {"graphs": 4096, "ms_per_step": r["ms_per_step"], "graphs_per_s": r["graphs_per_s"], "parameters": r["parameters"], "workload": r["workload"],
           "steps": 20, "warmup": 10}
    # Roofs of the step.  F_alg: the fp32 products of the reference's step -- per layer update_fn = Linear(d, 2d) + Linear(2d, d)
    # on N rows, the virtual node's mlp on G rows for all layers but the last, each product once forward and twice backward (input and weight
    # gradient).  B_alg: every activation the step must keep for its backward written once and read once, every gradient row written once and read
    # once, at 4 bytes: per layer x_in, the aggregated rows, the hidden rows before and after BatchNorm (2d wide), the output rows before and after
    # BatchNorm, plus the integer codes of the edges (7 columns of 8 bytes) and the parameters / their gradients three times (read, gradient, update).
    import re
    m = re.search(r"N=(\d+), E=(\d+)", r["workload"])
    if m:
        N, E, G, L, d = int(m.group(1)), int(m.group(2)), 4096, 5, 300
        f_alg = 3.0 * (L * 2.0 * N * (d * 2 * d * 2) + (L - 1) * 2.0 * G * (d * 2 * d * 2))
        rows_per_layer = N * (d + d + 2 * d + 2 * d + d + d)
        b_alg = 4.0 * 2.0 * 2.0 * L * rows_per_layer + 2.0 * L * E * 7 * 8.0 + 3.0 * 4.0 * r["parameters"]
        t = r["ms_per_step"] * 1e-3
        out["roofline"] = {"F_alg_GF": round(f_alg / 1e9, 1), "B_alg_GB": round(b_alg / 1e9, 3),
                           "fp32_equivalent_TFLOPs": round(f_alg / t / 1e12, 1), "frac_of_fp32_mfma_peak_157TF": round(f_alg / t / 1e12 / 157.3, 3),
                           "frac_of_fp16x3_roof_833TF": round(f_alg / t / 1e12 / 833.0, 3),
                           "hbm_GBs": round(b_alg / t / 1e9, 1), "hbm_frac": round(b_alg / t / 1e9 / HBM_PEAK_GBS, 3),
                           "roof_ms": {"hbm": round(b_alg / (HBM_PEAK_GBS * 1e9) * 1e3, 3), "fp16x3": round(f_alg / 833e12 * 1e3, 3)},
                           "note": "bound: neither single roof -- a sequence of ~440 launches per step, the dense ones on the matrix pipe (three fp16 plane products "
                                   "each; since r06 the weight gradients too, on the planes the forward and input-gradient products leave behind: "
                                   "gsn_wgrad_f16x3_hip), the BatchNorm passes writing those planes instead of fp32 rows (gsn_bn_act_planes_hip, "
                                   "gsn_bn_act_bwd_planes_hip), the row-wise ones at the HBM copy ceiling (profiles/r06_molhiv_step_kernel_stats.csv)"}
    return out


def train_small_batch(dev, graphs=True):
    """The reference's own batch sizes (README.md:121: molhiv 32 graphs; :112: ZINC 128): the whole training step eager and replayed as ONE
    HIP graph (gsn_amd.graphs.GraphedTrainStep: forward, native adjoints, gradient bucket, optimizer update).  Supplementary."""
    import importlib.util
    import types
    out = {}
    for name, batch in (("train_step_molhiv", 32), ("train_step_zinc", 128)):
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scripts", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        ent = {}
        for graph in ((False, True) if graphs else (False,)):
            r = mod.run(types.SimpleNamespace(batch=batch, steps=100, warmup=30, layers=5, d=300, graph=graph, optimizer="sgd"), dev)
            ent["hip_graph" if graph else "eager"] = {"ms_per_step": r["ms_per_step"], "graphs_per_s": r["graphs_per_s"]}
        ent["workload"] = r["workload"]
        out[name.replace("train_step_", "") + "_b%d" % batch] = ent
    return out


def count_er128(dev):
    """BASELINE configs[4]: counting only, Erdos-Renyi G(128, 1000) graphs x the 21 connected five-vertex patterns (58 vertex-orbit
    columns, non-induced), graphs per second of one launch of 2 048 and of 8 192 graphs (scripts/bench_counting_er.py is the stand-alone /
    multi-GPU form)."""
    import torch
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "orbits.npz"))
    pats = [z["all_simple_graphs_5/%d/edges" % i].tolist() for i in range(21)]
    plan = CountPlan.get(pats, "vertex", False)
    # (one workgroup per graph.  A launch costs ~10.5 ms + 14.6 us per graph: the search tails of the last workgroups are a fixed price, so the
    #  figure depends on the launch size -- 512 graphs 25 k/s, 2 048 53.5 k/s, 8 192 63 k/s, 32 768 66.5 k/s (scripts/bench_counting_er.py);
    #  BASELINE's 100 000 graphs are a few launches of the larger sizes, the 2 048-graph launch is kept as the figure of rounds 4-6)
    G_ALL, G = 8192, 2048
    b = synth.collate([synth.er_graph(128, 1000, s) for s in range(G_ALL)])
    node_ptr, edge_ptr = torch.from_numpy(b.node_ptr).to(dev), torch.from_numpy(b.edge_ptr).to(dev)
    ei = torch.from_numpy(b.edge_index).to(dev)
    out = torch.empty((b.num_nodes, plan.n_cols), dtype=torch.int64, device=dev)
    me = int(np.diff(b.edge_ptr).max())

    from gsn_amd import dist as gdist
    cost = np.asarray(gdist.counting_cost(b.edge_index, b.edge_ptr, 5), dtype=np.float64)

    def timed(g, reps):
        n_nodes = int(b.node_ptr[g])
        # (graphs handed out by falling estimated cost, sum_v deg^4: the long searches start first -- 53.3 k -> 55.1 k graphs/s at 2 048 graphs,
        #  scripts/gpu/r6_er_order.py; gsn_amd.dataset.prepare_graphs does the same)
        order = torch.from_numpy(np.argsort(-cost[:g], kind="stable").astype(np.int32)).to(dev)
        f = lambda: count_batch(plan, node_ptr[:g + 1], edge_ptr[:g + 1], ei, ids_are_global=True, max_nodes=128, max_edges=me, device=dev, out=out[:n_nodes], check=False,
                                graph_ids=order)
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, float(out[:n_nodes].sum().item())
    dt, occ = timed(G, 3)
    dt_all, occ_all = timed(G_ALL, 2)
    return {"graphs": G, "ms_per_launch": round(dt * 1e3, 3), "graphs_per_s": round(G / dt, 1), "columns": int(plan.n_cols),
            "occurrence_positions_per_s": round(occ / dt, 1),
            "launch_of_8192_graphs": {"graphs": G_ALL, "ms_per_launch": round(dt_all * 1e3, 3), "graphs_per_s": round(G_ALL / dt_all, 1),
                                      "occurrence_positions_per_s": round(occ_all / dt_all, 1),
                                      "note": "the same kernel on a larger launch: ~10.5 ms of search tails per launch + 14.6 us per graph (32 768 graphs: 66.5 k graphs/s)"}}


def linear_d300(dev):
    """The d = 300 node-level dense stage of the ogb layers (196 608 x 300 -> 600, gsn_linear_f16x3_fwd_hip incl. its row pre-pass) against
    the roofs of the pipe it uses: 2.5 PF/s fp16 / 3 plane products = 833 TF/s fp32-equivalent, and 8 TB/s on its algorithmic bytes."""
    import torch
    from gsn_amd import flags, layers
    M, K, Nn = 196608, 300, 600
    x = torch.randn(M, K, device=dev)
    W = torch.randn(Nn, K, device=dev) / K ** 0.5
    bb = torch.randn(Nn, device=dev)
    st = layers._Stage(W, bb, None, "relu", [(x, None)])
    spin_up(lambda: layers._launch_stages([st], M))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        layers._launch_stages([st], M)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    tf = 2.0 * M * K * Nn / ms / 1e9
    b_alg = 4.0 * (M * K + M * Nn + Nn * K)
    out = {"shape": [M, K, Nn], "ms": round(ms, 4), "fp32_equivalent_TFLOPs": round(tf, 1), "frac_of_fp16x3_roof_833TF": round(tf / (MFMA_BF16_PEAK_TF / 3.0), 4),
           "algorithmic_bytes": round(b_alg), "hbm_frac": round(b_alg / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)}
    # r06: what a TRAINING step runs at this shape -- the product over rows split earlier (the BatchNorm pass in front of it wrote the planes:
    # gsn_bn_act_planes_hip) and the weight gradient on the planes of X and gH (gsn_wgrad_f16x3_hip), beside the r05 weight gradient (gsn_wgrad_hip)
    try:
        from gsn_amd import _abi
        from gsn_amd._dense import _f16x3_weights
        L = _abi.lib()
        planes, col_inv = _f16x3_weights(W, W)
        y = torch.empty(M, Nn, device=dev)
        gh = torch.randn(M, Nn, device=dev) * 1e-4
        one = (_abi.gsn_block * 1)()

        def split(t):
            sc = torch.empty(int(L.gsn_linear_f16x3_scratch_bytes(t.shape[0], t.shape[1])), dtype=torch.uint8, device=dev)
            one[0].data = t.data_ptr(); one[0].idx = None; one[0].idx32 = None; one[0].width = t.shape[1]
            _abi.check(L.gsn_linear_f16x3_split_rows_hip(t.shape[0], 1, one, sc.data_ptr(), _abi.current_stream()), "gsn_linear_f16x3_split_rows_hip")
            return sc
        sx, sg = split(x), split(gh)
        gw = torch.zeros(Nn, K, device=dev)
        one[0].data = x.data_ptr(); one[0].width = K

        def timed(fn):
            spin_up(fn)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 10
        ms_pre = timed(lambda: _abi.check(L.gsn_linear_f16x3_fwd_presplit_hip(M, 1, one, planes.data_ptr(), col_inv.data_ptr(), bb.data_ptr(), Nn, None, None, None, 1,
                                                                                sx.data_ptr(), y.data_ptr(), _abi.current_stream()), "presplit"))
        ms_w16 = timed(lambda: _abi.check(L.gsn_wgrad_f16x3_hip(M, Nn, K, sg.data_ptr(), sx.data_ptr(), gw.data_ptr(), _abi.current_stream()), "wgrad16"))
        ms_w = timed(lambda: _abi.check(L.gsn_wgrad_hip(M, Nn, gh.data_ptr(), 1, one, gw.data_ptr(), _abi.current_stream()), "wgrad"))
        gf = 2.0 * M * K * Nn / 1e9
        out["rows_split_earlier"] = {"ms": round(ms_pre, 4), "fp32_equivalent_TFLOPs": round(gf / ms_pre, 1), "frac_of_fp16x3_roof_833TF": round(gf / ms_pre / (MFMA_BF16_PEAK_TF / 3.0), 4),
                                     "note": "gsn_linear_f16x3_fwd_presplit_hip: the product alone, rows split by the producer of the rows (r06 training path)"}
        out["weight_gradient_same_shape"] = {"planes_ms": round(ms_w16, 4), "planes_fp32_equivalent_TFLOPs": round(gf / ms_w16, 1),
                                             "bf16x6_ms": round(ms_w, 4), "bf16x6_fp32_equivalent_TFLOPs": round(gf / ms_w, 1),
                                             "note": "gsn_wgrad_f16x3_hip on the two row scratches vs gsn_wgrad_hip on fp32 rows (profiles/r06_wgrad16_phase.txt)"}
    except Exception as ex:  # noqa: BLE001
        out["rows_split_earlier"] = {"error": str(ex)[:200]}
    return out


def headline_line(world, G, N, E, args, dt):
    """The fields of the result line that a plain run and a --full run share (`dt`: the K timed steps, slowest rank)."""
    return {
        "metric": "graphs/sec (orbit-count + GSN-e fwd), ZINC-shape batch; % HBM roofline",
        "value": round(world * G * args.steps / dt, 1), "unit": "graphs/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "int64 counts + f32 message passing (matrix products: fp16x3 -- two fp16 planes per fp32 operand, three plane products, f32 accumulate)", "data": "synthetic",
        "config": {"workload": "ZINC-shape x%d graphs/GPU (N=%d, E=%d): integer atom / bond codes in -> cycle_graph k<=6 GSN-e (id_scope=local) "
                               "orbit count (int64 identifiers written) + one-hot encoding (atoms, bonds and identifiers as exact fp16 operand rows: the layer kernel's "
                               "input form; no fp32 one-hot tensor is materialised) + GSN_edge_sparse layer-0 forward (general, d_in=28, "
                               "d_ef=4, d_id=12, d=128, bn, eval) -> layer rows out" % (G, N, E),
                   "inputs": "int64 atom codes [N], bond codes [E], edge_index [2, E], graph pointers", "outputs": "int64 identifiers [E, 4], fp32 layer rows [N, 128]",
                   "graphs_per_step_per_gpu": G, "parallelism": "graph-shard x%d, no data-path collective" % world},
        "full": bool(args.full),
    }


DUMP_ROWS = 65536       # rows per output that --dump-outputs writes (a fixed seeded sample where the output has more)


def dump_outputs(out_dir, ids, y):
    """--dump-outputs: what the last timed step hands its caller -- the int64 identifiers [E, 4] and the layer rows [N, 128] -- as
    <name>.npy (DUMP_ROWS rows drawn with a fixed seed, in row order; identifiers as float64, exact), <name>_rows.npy (the row numbers
    drawn) and <name>_colsum.npy (float64 column sums over ALL rows).  About 35 MB at the default batch."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    for name, t in (("identifiers", ids), ("layer_rows", y)):
        n = t.shape[0]
        rows = np.arange(n) if n <= DUMP_ROWS else np.sort(np.random.default_rng(0).choice(n, DUMP_ROWS, replace=False))
        sample = t[torch.from_numpy(rows).to(t.device)].cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), sample.astype(np.float64 if t.dtype == torch.int64 else np.float32))
        np.save(os.path.join(out_dir, name + "_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(out_dir, name + "_colsum.npy"), t.sum(0, dtype=torch.float64).cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=65536, help="graphs per step per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also the checks and supplementary measurements: oracle comparison of the timed batch, per-kernel times and roofline, "
                         "HIP-graph replays, step variants, other sizes / configurations, RCCL all-reduce, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (identifiers and layer rows: a fixed seeded sample) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the supplementary measurements (profiling runs: only the headline launches)")
    ap.add_argument("--no-graph", action="store_true", help="with --full: skip the HIP-graph replay of the timed steps (eager launches only)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="process-group backend (nccl = RCCL; gloo only with --dry-run)")
    ap.add_argument("--dry-run", action="store_true",
                    help="plumbing check without a GPU: launch, rendezvous, barrier, max-over-ranks and the JSON line run for real, "
                         "the step is an empty stub (the line carries dry_run=true and no throughput claim)")
    args = ap.parse_args()

    from gsn_amd import dist as gdist
    if args.gpus > 1 and not gdist.under_launcher():
        # `python bench.py --gpus N`: start the N ranks ourselves (one per GPU, torch.distributed.run, rendezvous on
        # 127.0.0.1); under the driver's own `python -m torch.distributed.run ... bench.py --gpus N` this is skipped.
        raise SystemExit(gdist.launch_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:]))

    import torch
    if args.dry_run:
        return dry_run(args)
    import networkx as nx
    from gsn_amd import flags, layers
    from gsn_amd.counting import CountPlan, count_batch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the hot path is HIP-only; there is no CPU fallback)")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gdist.require_devices(max(int(os.environ.get("LOCAL_WORLD_SIZE", "1")), local_rank + 1))     # (fails loudly, before any collective)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # launched by torch.distributed.run (also with one process): RCCL is used for the barrier and the max-over-ranks only
    rank, world, local_rank, dist = gdist.init_from_env("nccl", dev)
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks" % (args.gpus, world))

    G = args.graphs
    b = make_batch(G, seed=1000 + rank)       # every rank owns a different shard of graphs
    N, E = b.num_nodes, b.num_edges
    max_nodes = int(np.diff(b.node_ptr).max())
    max_edges = int(np.diff(b.edge_ptr).max())
    node_ptr = torch.from_numpy(b.node_ptr).to(dev)
    edge_ptr = torch.from_numpy(b.edge_ptr).to(dev)
    ei = torch.from_numpy(b.edge_index).to(dev)
    x = torch.nn.functional.one_hot(torch.from_numpy(b.atom_type), 28).float().to(dev)
    ef = torch.nn.functional.one_hot(torch.from_numpy(b.bond_type), 4).float().to(dev)
    degrees = torch.zeros(N, device=dev)
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    plan.device_table(dev)
    ids_out = torch.empty((E, plan.n_cols), dtype=torch.int64, device=dev)
    idf_out = torch.empty((E, 12), dtype=torch.float32, device=dev)    # the encoded identifiers the layer reads
    torch.manual_seed(0)
    layer = layers.GSN_edge_sparse(**CTOR).to(dev).eval()

    # high priority: the CSR kernels are short and memory-bound; at equal priority their workgroups queue behind the
    # counting kernel's and the build (0.13 ms alone) stretches past the end of the counting (GSN_SIDE_PRIO=0 to compare)
    side = torch.cuda.Stream(device=dev, priority=-1 if os.environ.get("GSN_SIDE_PRIO", "1") != "0" else 0)
    sel = layer._sel()
    # the batch's graph boundaries (the pointers the counting kernel takes as well): the layer's target-sorted CSR is then built by
    # ONE launch, every graph sorted in LDS (gsn_csr_build_graphs_hip), instead of the generic seven
    if os.environ.get("GSN_BENCH_GENERIC_CSR", "0") == "0":
        layers.set_graph_partition(ei, node_ptr, edge_ptr, max_nodes, max_edges, check=False)

    # Exact fp16 row packs (gsn_amd.packs): every input of this layer is a one-hot encoding, exact in fp16.  The static inputs (x, bond
    # types) get their packs where their fp32 one-hot rows are made -- once, outside the timed region, like those rows themselves; the
    # identifiers' columns are written by the counting kernel inside the timed step, next to the fp32 rows it writes anyway.  The layer
    # then runs csrc/layer_rp.hip (same arithmetic, no fp32 -> fp16 conversion of its gathered rows).  GSN_BENCH_PACK16=0: the fp32-row
    # kernel (csrc/layer_rr.hip), reported beside the headline as kernels.layer_fp32_rows either way.
    from gsn_amd import packs
    use_pack = os.environ.get("GSN_BENCH_PACK16", "1") != "0" and os.environ.get("GSN_FUSED_RR", "1") != "0"
    epack = None
    if use_pack:
        packs.node_pack(x, check=True)
        epack = packs.new_edge_pack(E, dev)
        packs._pack_rows(ef, epack, 12, -1, True)
        packs.claim(ef, epack, 12)

    # The headline step takes what the reference path takes and leaves what it leaves: integer atom / bond codes in
    # (utils_graph_learning.py:170-187 encodes them inside the model), int64 substructure identifiers (utils_ids.py:19-27) AND the layer's
    # output rows out.  Atom and bond codes go straight into exact fp16 row packs (gsn_one_hot_pack16_hip) inside the step, on the side
    # stream under the counting kernel; the counting kernel writes the int64 identifiers, their one-hot rows and the packs' identifier
    # columns.  `prepacked=True` is the step of rounds 2-4 (dense one-hot inputs and their packs made outside the step, no int64
    # identifiers written): reported as kernels.step_prepacked.
    xc = layers.Codes(torch.from_numpy(b.atom_type).to(dev), [28])
    efc = layers.Codes(torch.from_numpy(b.bond_type).to(dev), [4])
    flags.CODE_STATUS_CHECK = False          # atom / bond codes are in range by construction, counts are clamped
    epack_c = packs.new_edge_pack(E, dev) if use_pack else None
    npack_c = packs.new_node_pack(N, dev) if use_pack else None

    # r06: the headline step is ONE host call and TWO kernel launches (gsn_amd.step.CountLayerStep -> gsn_count_layer_step_hip): the counting
    # launch, whose side workgroups also sort the batch into the layer's CSR and encode the atom / bond codes into the packs, then the layer.
    # GSN_BENCH_ONE_CALL=0: the six-launch composition of r05 (CSR build + two code encoders on a second stream under the counting kernel),
    # reported beside the headline as kernels.step_six_launches either way.
    from gsn_amd.step import CountLayerStep
    one_call = use_pack and PACK_ONLY_IDS and os.environ.get("GSN_BENCH_ONE_CALL", "1") != "0"
    stepper = CountLayerStep(plan, layer, [3, 3, 3, 3], clamp=True) if one_call else None

    def step(fork=True, int64_ids=True, prepacked=not use_pack, six=not one_call):
        if not six:
            return stepper(node_ptr, edge_ptr, ei, xc, efc, max_nodes, max_edges, ids_out=ids_out)[1]
        layers._CSR_CACHE.clear()             # the CSR of a fresh batch is part of the forward pass
        main = torch.cuda.current_stream(dev)
        ep = epack if prepacked else epack_c

        ids_in = [idf_out]

        def count():
            # the counts leave the kernel as the int64 identifiers AND as the one-hot classes of min(count, 2) the layer consumes (the
            # reference: int64 identifiers, then DiscreteEmbedding('one_hot_encoder'), utils_graph_learning.py:78 / :170-187).  Headline:
            # int64 rows + the identifier columns of the exact fp16 pack the layer kernel reads (gsn_count_encode_pack16_hip with no fp32
            # rows: nothing reads them -- the layer input is a Codes object over the counts, tagged with the pack); the other variants
            # write the fp32 one-hot rows as rounds 2-4 did
            pack_only = use_pack and int64_ids and not prepacked and PACK_ONLY_IDS
            with layers._timed("count", 16.0 * E + (2.0 if pack_only else 4.0) * E * 12 + (8.0 * E * 4 if int64_ids else 0.0)):
                if pack_only:
                    ids_in[0] = count_batch(plan, node_ptr, edge_ptr, ei, ids_are_global=True, max_nodes=max_nodes, max_edges=max_edges,
                                            device=dev, check=False, encode=([3, 3, 3, 3], True), counts=True, out=ids_out,
                                            encoded_pack=(ep, 0), encoded_rows=False)[2]
                else:
                    count_batch(plan, node_ptr, edge_ptr, ei, ids_are_global=True, max_nodes=max_nodes, max_edges=max_edges,
                                device=dev, check=False, encode=([3, 3, 3, 3], True), counts=int64_ids, out=ids_out if int64_ids else None,
                                encoded_out=idf_out, encoded_pack=(ep, 0) if use_pack else None)

        def independent_of_counts():
            layers._csr_for(ei, sel, N)
            if not prepacked:
                packs.pack_node_codes(xc, npack_c)
                packs.pack_edge_codes(efc, epack_c, 12)

        def run_layer():
            with torch.no_grad():
                if prepacked:
                    return layer(x, ei, identifiers=idf_out, degrees=degrees, edge_features=ef)
                return layer(xc, ei, identifiers=ids_in[0], degrees=degrees, edge_features=efc)
        if not fork:                          # (the captured variant without a second branch)
            independent_of_counts()
            count()
            return run_layer()
        # The layer's target-sorted CSR depends only on edge_index, the atom / bond packs only on the codes, the counting only on the graphs:
        # the former (small memory-bound kernels) run on a second HIP stream under the VALU-bound counting kernel.  The side stream first
        # waits for the main stream so that buffers recycled by the allocator are no longer read by the previous step.
        side.wait_stream(main)
        with torch.cuda.stream(side):
            independent_of_counts()
        count()
        main.wait_stream(side)
        return run_layer()

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def diag(tag):
        if not os.environ.get("GSN_BENCH_DIAG_ORDER"):
            return
        for _ in range(3):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        print("diag position %s: %.4f ms" % (tag, (time.perf_counter() - t0) / args.steps * 1e3), file=sys.stderr)

    # untimed, before the W warm-up steps: first-launch costs and the GPU clock ramp after the idle host-side data generation
    # (the device needs ~0.1 s of load to reach its steady state: 5 steps 1.44 ms/step, 60 steps 1.39; GSN_BENCH_PREWARM)
    for _ in range(int(os.environ.get("GSN_BENCH_PREWARM", "60"))):
        step()
    for _ in range(args.warmup):
        step()
    sync()
    diag("before the timed region")
    diag("before the timed region, again")
    # HIP events inside the timed region bracket the DOMINANT kernel only (the layer: `roofline.avg_launch_ms`); the full per-kernel breakdown
    # (`ms_per_step_by_kernel`) comes from K more steps right behind the timed region, bracketed everywhere (an event pair around every launch
    # keeps consecutive kernels from overlapping their ends: ~1 % of the step).
    # (a plain run brackets nothing: the events only feed the per-kernel figures of --full)
    if args.full:
        flags.KERNEL_TIMER = {}
        flags.KERNEL_TIMER_ONLY = {"layer_fused"} if os.environ.get("GSN_BENCH_NO_EVENTS", "0") == "0" else set()      # (diagnostic: no event at all)
    import gc
    _dm = os.environ.get("GSN_BENCH_DIAG_MODE", "")
    if "collect" in _dm:                      # (diagnostic: a collection here frees blocks and changes where the step's buffers land -- 0.754 -> 0.854 ms)
        gc.collect()
    gc.disable()                              # (the timed region is ~16 ms: one collector pause of the interpreter would be a tenth of it)
    if "empty" in _dm:
        torch.cuda.empty_cache()
        for _ in range(10):
            step()
        sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if "drop" in _dm:
            step()
            continue
        y = step()
    t_enq = time.perf_counter() - t0          # host time to enqueue the K steps (the GPU runs behind it)
    sync()
    dt = time.perf_counter() - t0
    gc.enable()
    if "drop" in _dm:
        y = step()
        sync()
    if args.dump_outputs and rank == 0:      # (before any further step: the step's buffers are reused)
        dump_outputs(args.dump_outputs, ids_out, y)
    if not args.full:
        dt_own = dt
        dt = gdist.max_over_ranks(dt, dev)
        assert torch.isfinite(y).all()
        per_rank_ms, graphs_by_rank = [round(dt_own / args.steps * 1e3, 4)], [G]
        if dist is not None and world > 1:
            tl = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(tl, torch.tensor([dt_own], device=dev, dtype=torch.float64))
            per_rank_ms = [round(float(t.item()) / args.steps * 1e3, 4) for t in tl]
            gl = [torch.zeros(1, device=dev, dtype=torch.int64) for _ in range(world)]
            dist.all_gather(gl, torch.tensor([G], device=dev, dtype=torch.int64))
            graphs_by_rank = [int(t.item()) for t in gl]
        if rank == 0:
            res = headline_line(world, G, N, E, args, dt)
            res["kernels"] = {"ms_per_step_by_rank": per_rank_ms, "graphs_by_rank": graphs_by_rank,
                              "host_enqueue_ms_per_step": round(t_enq / args.steps * 1e3, 4),
                              "prewarm_steps_untimed": int(os.environ.get("GSN_BENCH_PREWARM", "60"))}
            print(json.dumps(res))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    timer_dom, flags.KERNEL_TIMER, flags.KERNEL_TIMER_ONLY = flags.KERNEL_TIMER, {}, None
    for _ in range(args.steps):              # (untimed: the same K steps with every kernel family bracketed)
        step()
    sync()
    timer, flags.KERNEL_TIMER = flags.KERNEL_TIMER, None
    timer["layer_fused"] = timer_dom.get("layer_fused", timer.get("layer_fused", []))      # the dominant kernel's events are those of the TIMED steps
    dt_own = dt
    dt = gdist.max_over_ranks(dt, dev)
    assert torch.isfinite(y).all()
    print("diag timed region: %.4f ms" % (dt / args.steps * 1e3), file=sys.stderr) if os.environ.get("GSN_BENCH_DIAG_ORDER") else None
    diag("right behind the timed region")
    # (outside the timed region) the timed batch's own results against the oracle, and the counting work figures: the int64
    # counts of the same batch (one more launch), the timed step's encoded rows against their one-hot, a tile against the oracle
    ids_timed = ids_out.clone()               # (the int64 identifiers the timed step wrote)
    count_batch(plan, node_ptr, edge_ptr, ei, ids_are_global=True, max_nodes=max_nodes, max_edges=max_edges, device=dev, out=ids_out, check=False)
    one_hot_ref = torch.nn.functional.one_hot(ids_out.clamp(max=2), 3).reshape(E, 12).float()
    ids_ok = bool(torch.equal(ids_timed, ids_out))
    side_ok = None
    if one_call:                              # the packs and the CSR the timed step's counting launch wrote: against the encoders' definition / the CSR entry point
        npk_t, epk_t = stepper.packs()
        enc_ok = bool(torch.equal(epk_t[:, :12].float(), one_hot_ref))
        csr_t = stepper.csr()
        from gsn_amd._index import build_csr_graphs
        seg_r, perm_r, tgt_r, src_r = build_csr_graphs(ei[sel], N, node_ptr, edge_ptr, max_nodes, max_edges, other=ei[1 - sel], check=True)
        side_ok = {"edge_pack_bond_columns_equal_one_hot_of_codes": bool(torch.equal(epk_t[:, 12:].float(), torch.nn.functional.one_hot(efc.codes[:, 0], 4).float())),
                   "node_pack_equals_one_hot_of_codes": bool(torch.equal(npk_t[:, :28].float(), torch.nn.functional.one_hot(xc.codes[:, 0], 28).float())
                                                              and bool((npk_t[:, 28:31] == 0).all()) and bool((npk_t[:, 31] == 1).all())),
                   "csr_arrays_bit_equal_to_gsn_csr_build_graphs_hip": bool(torch.equal(csr_t.seg_ptr, seg_r) and torch.equal(csr_t.perm[:E], perm_r)
                                                                             and torch.equal(csr_t.tgt[:E], tgt_r) and torch.equal(csr_t.src[:E], src_r))}
        assert all(side_ok.values()), "side outputs of the timed step: %r" % (side_ok,)
    elif use_pack and PACK_ONLY_IDS:          # the timed step's identifier columns of the pack (fp16, exact) against one_hot(min(count, 2))
        enc_ok = bool(torch.equal(epack_c[:, :12].float(), one_hot_ref))
    else:
        enc_ok = bool(torch.equal(idf_out, one_hot_ref))
    assert enc_ok and ids_ok, "identifiers of the timed step differ from a plain counting launch / its encoded form from one_hot(min(count, 2))"
    checked = verify_tile(plan, b, ids_out, y, layer, 4096) if rank == 0 else None
    if checked is not None:
        checked["encoded_rows_equal_one_hot_of_counts"] = enc_ok
        checked["int64_identifiers_of_the_timed_step_equal_a_plain_counting_launch"] = ids_ok
        if side_ok is not None:
            checked.update(side_ok)
    occ_pos, n_maps = work_figures([list(nx.cycle_graph(k).edges) for k in range(3, 7)], ids_out)

    diag("behind the oracle checks")
    # Diagnostic (never `value`): the same K steps replayed from ONE captured HIP graph of the step (same kernels, same inputs).
    dt_graph, graph_note, dt_graph_fork = None, None, None
    res_eager_late = {}
    if not args.no_graph:
        # two captures: the step as it runs eagerly (CSR build forked onto the side stream: two branches in the graph) and the same
        # kernels in one chain.  hipGraph runs the branches of the forked capture on its own internal streams without the side stream's
        # priority, and the join costs a cross-stream signal each way: measured 1.02 ms forked vs 0.81 eager in round 3.
        res_g, res_eager_late = {}, {}
        for tag, fork in ((("chain", False),) if one_call else (("fork", True), ("chain", False))):
            ok = 1
            try:
                gobj = torch.cuda.CUDAGraph()
                cap = torch.cuda.Stream(device=dev)
                cap.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(cap):
                    step(fork=fork)
                torch.cuda.current_stream(dev).wait_stream(cap)
                with torch.cuda.graph(gobj):
                    y_g = step(fork=fork)
                for _ in range(int(os.environ.get("GSN_BENCH_PREWARM", "60"))):      # (the oracle checks above idled the GPU: clocks, as in front of the timed region)
                    gobj.replay()
                sync()
                if not (torch.isfinite(y_g).all() and torch.allclose(y_g, y, rtol=1e-4, atol=1e-5)):
                    raise RuntimeError("graph replay output differs from the eager step")
            except Exception as e:       # capture is best effort
                ok, graph_note = 0, "capture failed: " + str(e)[:160]
            if dist is not None:         # every rank takes the same branch
                f = torch.tensor([ok], device=dev, dtype=torch.int32)
                dist.all_reduce(f, op=dist.ReduceOp.MIN)
                ok = int(f.item())
            if ok:
                # eager steps and replays timed ALTERNATELY, right here: behind the oracle checks the clocks are not those of the timed region
                # (the same eager steps read 8-11 % slower at this point of the run), and the two must be compared like for like
                pairs = []
                for _ in range(3):
                    rec = []
                    for fn in ((lambda: step(fork=fork)), gobj.replay):
                        for _ in range(10):
                            fn()
                        sync()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            fn()
                        sync()
                        rec.append(gdist.max_over_ranks(time.perf_counter() - t0, dev))
                    pairs.append(rec)
                best = min(pairs, key=lambda r: r[1])
                res_g[tag] = best[1]
                res_eager_late[tag] = best[0]
            del gobj
        dt_graph_fork = res_g.get("fork")
        dt_graph = min(res_g.values()) if res_g else None
    dt_eager = dt      # the headline is the eager timing, always; the graph replays are diagnostics

    # Supplementary (never `value`): the step of rounds 2-4 -- dense one-hot inputs and their packs made OUTSIDE the step, no int64
    # identifiers written (E x 4 x 8 bytes less) -- and the headline step without the int64 identifiers.
    dt_pre = dt_noids = dt_six = t_enq_six = None
    if one_call:
        for _ in range(30):
            step(six=True)
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(six=True)
        t_enq_six = time.perf_counter() - t0
        sync()
        dt_six = gdist.max_over_ranks(time.perf_counter() - t0, dev)
    if use_pack:
        for kw in ({"prepacked": True, "int64_ids": False, "six": True}, {"int64_ids": False, "six": True}):
            for _ in range(3):
                step(**kw)
            sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(**kw)
            sync()
            t_kw = gdist.max_over_ranks(time.perf_counter() - t0, dev)
            if kw.get("prepacked"):
                dt_pre = t_kw
            else:
                dt_noids = t_kw

    if os.environ.get("GSN_BENCH_DIAG_ORDER"):       # (diagnostic: the two step variants timed alternately, keeping / dropping the output)
        for tag, kw, keep in (("A keep", {}, True), ("B", {"int64_ids": False}, False), ("A drop", {}, False), ("B keep", {"int64_ids": False}, True), ("A keep", {}, True)):
            for _ in range(3):
                step(**kw)
            sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                if keep:
                    y = step(**kw)
                else:
                    step(**kw)
            sync()
            print("diag %s: %.4f ms" % (tag, (time.perf_counter() - t0) / args.steps * 1e3), file=sys.stderr)

    # Supplementary: the layer alone, back to back, on its fp16 packs (the timed step's kernel) and on the fp32 rows (csrc/layer_rr.hip)
    layer_alone = {}
    if world == 1 and not args.no_extras:
        if use_pack:
            step(prepacked=True, int64_ids=False, six=True)      # (the dense tensors' pack tags all point at one edge pack again)
        with torch.no_grad():
            for tag in (("pack16_rows", "fp32_rows") if use_pack else ("fp32_rows",)):
                if tag == "fp32_rows":
                    saved = [(t, getattr(t, "_gsn_pack16", None)) for t in (x, ef, idf_out)]
                    for t, _ in saved:
                        packs.release(t)
                for _ in range(10):
                    layer(x, ei, identifiers=idf_out, degrees=degrees, edge_features=ef)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(30):
                    layer(x, ei, identifiers=idf_out, degrees=degrees, edge_features=ef)
                e1.record()
                torch.cuda.synchronize()
                layer_alone[tag] = round(e0.elapsed_time(e1) / 30, 4)
                if tag == "fp32_rows":
                    for t, tg in saved:
                        t._gsn_pack16 = tg

    fused = None

    # Supplementary (never `value`): count + the FULL model of BASELINE configs[1] (GNNSubstructures, 4 layers: layer 0 is
    # GSN_edge_sparse, layers 1-3 MPNN_edge_sparse with K = 260 edge rows -- the any-shape dense kernels; one-hot encoders, sum
    # readout, eval) on the same batch.
    model4 = None
    if world == 1 and not args.no_extras:
        try:
            step_model, gm = full_model_closure(dev, min(G, 16384), batch=(b, node_ptr, edge_ptr, ei, plan, max_nodes, max_edges))
            ym = step_model()
            spin_up(step_model)
            t3 = time.perf_counter()
            for _ in range(args.steps):
                ym = step_model()
            torch.cuda.synchronize()
            dt3 = time.perf_counter() - t3
            model4 = {"graphs_per_s": round(gm * args.steps / dt3, 1), "ms_per_step": round(dt3 / args.steps * 1e3, 4), "graphs_per_step": gm,
                      "finite": bool(torch.isfinite(ym).all()),
                      "note": "count + GNNSubstructures eval forward (4 layers d=128, one-hot encoders, jk, sum readout) on %d graphs" % gm}
            del step_model
        except Exception as ex:      # supplementary: never fails the headline
            model4 = {"error": str(ex)[:200]}

    # Supplementary (never `value`): the same step on the dataset size of BASELINE configs[1] (ZINC-12k: 12 000 graphs,
    # one launch sequence for the whole dataset; the working set sits in the 256 MB Infinity Cache at this size).
    zinc12k = None
    if world == 1 and G != 12000 and not args.no_extras:
        b2 = make_batch(12000, seed=77)
        np2, ep2 = torch.from_numpy(b2.node_ptr).to(dev), torch.from_numpy(b2.edge_ptr).to(dev)
        ei2 = torch.from_numpy(b2.edge_index).to(dev)
        x2 = torch.nn.functional.one_hot(torch.from_numpy(b2.atom_type), 28).float().to(dev)
        ef2 = torch.nn.functional.one_hot(torch.from_numpy(b2.bond_type), 4).float().to(dev)
        deg2 = torch.zeros(b2.num_nodes, device=dev)
        ids2 = torch.empty((b2.num_edges, plan.n_cols), dtype=torch.int64, device=dev)
        mn2, me2 = int(np.diff(b2.node_ptr).max()), int(np.diff(b2.edge_ptr).max())

        headline_flow = use_pack and PACK_ONLY_IDS
        if headline_flow:
            # the headline step's flow at this size: integer codes in, CSR + code packs on the side stream, int64 identifiers + pack columns from
            # the counting kernel, the packed-row layer kernel (rounds 1-4 and early r05 ran the r01 flow here: counts -> one-hot launch -> the
            # layer on dense fp32 rows)
            if os.environ.get("GSN_BENCH_GENERIC_CSR", "0") == "0":
                layers.set_graph_partition(ei2, np2, ep2, mn2, me2, check=False)
            xc2 = layers.Codes(torch.from_numpy(b2.atom_type).to(dev), [28])
            efc2 = layers.Codes(torch.from_numpy(b2.bond_type).to(dev), [4])
            npk2, epk2 = packs.new_node_pack(b2.num_nodes, dev), packs.new_edge_pack(b2.num_edges, dev)

        stepper2 = CountLayerStep(plan, layer, [3, 3, 3, 3], clamp=True) if (headline_flow and one_call) else None

        def step12k():
            if stepper2 is not None:
                return stepper2(np2, ep2, ei2, xc2, efc2, mn2, me2, ids_out=ids2)[1]
            layers._CSR_CACHE.clear()
            if headline_flow:
                # (one stream: at this size the step is 0.18 ms of GPU time and the second stream's events and waits make the HOST the
                #  bound -- 0.205 ms per step enqueued against 0.178 in one chain, scripts/gpu/z12k.py; from ~16 000 graphs on the fork wins)
                layers._csr_for(ei2, sel, b2.num_nodes)
                packs.pack_node_codes(xc2, npk2)
                packs.pack_edge_codes(efc2, epk2, 12)
                idc2 = count_batch(plan, np2, ep2, ei2, ids_are_global=True, max_nodes=mn2, max_edges=me2, device=dev, check=False,
                                   encode=([3, 3, 3, 3], True), counts=True, out=ids2, encoded_pack=(epk2, 0), encoded_rows=False)[2]
                with torch.no_grad():
                    return layer(xc2, ei2, identifiers=idc2, degrees=deg2, edge_features=efc2)
            count_batch(plan, np2, ep2, ei2, ids_are_global=True, max_nodes=mn2, max_edges=me2, device=dev, out=ids2, check=False)
            idf2 = layers.one_hot_identifiers(ids2, [3, 3, 3, 3], clamp=True)
            with torch.no_grad():
                return layer(x2, ei2, identifiers=idf2, degrees=deg2, edge_features=ef2)
        # the batch above was generated on the host while the GPU idled: warm up long enough for the clocks to come back
        # (a 0.6 ms step measured right after an idle phase reads anywhere between 0.6 and 2.5 ms)
        n12 = max(args.steps, 100)
        for _ in range(100):
            step12k()
        torch.cuda.synchronize()
        spin_up(step12k)
        t2 = time.perf_counter()
        for _ in range(n12):
            step12k()
        torch.cuda.synchronize()
        dt2 = time.perf_counter() - t2
        zinc12k = {"graphs_per_s": round(12000 * n12 / dt2, 1), "ms_per_step": round(dt2 / n12 * 1e3, 4), "steps": n12,
                   "note": "BASELINE configs[1] dataset size: 12 000 ZINC-shaped graphs per step (N=%d, E=%d); %s" % (
                       b2.num_nodes, b2.num_edges, "the headline step's flow (codes in, int64 identifiers + layer rows out)" if headline_flow
                       else "counts -> one-hot launch -> the layer on dense fp32 rows")}
        # the 12 000-graph step's layer rows against the headline kernel's on the same graphs would need a second oracle pass; its int64
        # identifiers are compared with a plain counting launch here
        ids12 = ids2.clone()
        count_batch(plan, np2, ep2, ei2, ids_are_global=True, max_nodes=mn2, max_edges=me2, device=dev, out=ids2, check=False)
        zinc12k["int64_identifiers_equal_a_plain_counting_launch"] = bool(torch.equal(ids12, ids2))

    # Supplementary (never `value`): the reference's real batch sizes, the stand-alone aggregation stage, the layer on real-valued inputs
    small = prop = flt = wide = train4 = lin300 = er128 = train_small = None
    if world == 1 and not args.no_extras:
        try:
            small = small_batch_steps(plan, layer, dev, graphs=not args.no_graph)
        except Exception as ex:
            small = {"error": str(ex)[:200]}
        try:
            prop = propagate_figures(b, dev)
        except Exception as ex:
            prop = {"error": str(ex)[:200]}
        try:
            flt = float_input_layer(layer, b, ei, dev)
        except Exception as ex:
            flt = {"error": str(ex)[:200]}
        try:
            wide = wide_layer(b, ei, dev)
        except Exception as ex:
            wide = {"error": str(ex)[:200]}
        try:
            train4 = train_step_config4(dev)
        except Exception as ex:
            train4 = {"error": str(ex)[:200]}
        try:
            train_small = train_small_batch(dev, graphs=not args.no_graph)
        except Exception as ex:
            train_small = {"error": str(ex)[:200]}
        try:
            lin300 = linear_d300(dev)
        except Exception as ex:
            lin300 = {"error": str(ex)[:200]}
        try:
            er128 = count_er128(dev)
        except Exception as ex:
            er128 = {"error": str(ex)[:200]}
    # every rank's own time of the K steps (the headline takes the maximum): a slow rank shows up by name in the N > 1 line
    per_rank_ms = [round(dt_own / args.steps * 1e3, 4)]
    if dist is not None and world > 1:
        tl = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tl, torch.tensor([dt_own], device=dev, dtype=torch.float64))
        per_rank_ms = [round(float(t.item()) / args.steps * 1e3, 4) for t in tl]

    # the collective that a data-parallel training step adds (the headline path has none): one flat gradient bucket of the configs[3]
    # model's size (3.35 M fp32 parameters, 13.4 MB) all-reduced over RCCL, timed on its own -- also at world size 1 under the launcher
    rccl = None
    graphs_by_rank = [G]
    if dist is not None:
        bucket = torch.zeros(3353406, dtype=torch.float32, device=dev)
        for _ in range(3):
            dist.all_reduce(bucket)
        sync()
        t0 = time.perf_counter()
        for _ in range(10):
            dist.all_reduce(bucket)
        sync()
        t_ar = gdist.max_over_ranks((time.perf_counter() - t0) / 10, dev)
        ranks = gdist.rank_report(dev)
        buses = [r.get("pci_bus_id") for r in ranks]
        rccl = {"version": ".".join(str(v) for v in torch.cuda.nccl.version()), "allreduce_ms": round(t_ar * 1e3, 4), "bucket_MB": 13.41,
                "allreduce_busbw_GBs": round(2.0 * (world - 1) / world * 13.41e-3 / t_ar, 1) if world > 1 else None,
                "world_size_reported": dist.get_world_size(), "backend": dist.get_backend(),
                "ranks": ranks, "distinct_devices": len(set(buses)) == len(buses) if all(b is not None for b in buses) else None,
                "note": "flat fp32 gradient bucket of the configs[3] model, sum over %d rank(s); not part of the headline step" % world}
        if world > 1 and rccl["distinct_devices"] is False:
            raise SystemExit("bench.py: two ranks share one GPU: %r" % (ranks,))
        gl = [torch.zeros(1, device=dev, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(gl, torch.tensor([G], device=dev, dtype=torch.int64))
        graphs_by_rank = [int(t.item()) for t in gl]

    if rank == 0:
        kernels = {}
        merged = {}
        for name, evs in timer.items():   # mlp_chain1 / mlp_chain2 (1- and 2-stage launches) are one kernel family
            merged.setdefault("mlp_chain" if name.startswith("mlp_chain") else name, []).extend(evs)
        per_launch = {name: round(sum(e0.elapsed_time(e1) for e0, e1, _ in evs) / args.steps, 4) for name, evs in timer.items()}
        for name, evs in merged.items():
            ms = [e0.elapsed_time(e1) for e0, e1, _ in evs]
            work = sum(w for _, _, w in evs)
            kernels[name] = {"launches_per_step": len(evs) / args.steps, "ms_per_step": sum(ms) / args.steps, "work_per_step": work / args.steps}
        fams = [k for k in ("layer_fused", "mlp_chain", "linear_fwd", "propagate_fwd", "count") if k in kernels]
        dom = max(fams, key=lambda k: kernels[k]["ms_per_step"])
        kd = kernels[dom]
        n_par = sum(p.numel() for p in layer.parameters())
        # the layer's compulsory traffic (every input once, the output once, no intermediates), edge_index as int64
        survey_b_alg = 16.0 * E + 4.0 * (N * 28.0 + E * 12.0 + E * 4.0 + N * 128.0 + n_par)
        if dom == "layer_fused":
            # ONE launch runs the whole layer.  Algorithmic bytes of THIS launch: the three int32 row-source arrays and seg_ptr of
            # the CSR (instead of the int64 edge_index, which the CSR build reads), x, identifiers, edge features, parameters, output.
            t_k = kd["ms_per_step"] / kd["launches_per_step"] * 1e-3
            b_launch = 12.0 * E + 4.0 * (N + 1) + 4.0 * (N * 28.0 + E * 12.0 + E * 4.0 + N * 128.0 + n_par)
            # matrix work actually executed on v_mfma_f32_32x32x16_f16: fp16x3 (three plane products per fp32 product; two in the
            # edge stage here, whose one-hot input rows are exact in fp16)
            f_alg = 2.0 * E * 72 * 128 + 2.0 * N * ((28 + 128 + 1) * 128 + 128 * 128)
            # executed v_mfma_f32_32x32x16_f16 instructions of csrc/layer_rr.hip (32 768 flop each), from the tiles and 32-row edge
            # blocks its iterator forms on this batch: per block 5 x 4 x 2 products of the edge stage (input rows exact in fp16: two
            # plane products) + 2 x 4 x 2 of the incidence product that sums the activated rows per target (two fp16 planes); per
            # tile (10 + 8) x 4 x 3 of the two node stages.  (GSN_FUSED_RR=0: layer_fused.hip, 2 / 3 products per fp32 product, no
            # incidence product.)
            rr = os.environ.get("GSN_FUSED_RR", "1") != "0"
            if rr:
                n_t, n_b = rr_tiling((stepper.csr() if one_call else layers._csr_for(ei, sel, N)).seg_ptr.cpu().numpy().astype(np.int64), N)
                # (csrc/layer_rp.hip: the x part of node stage 0 is exact as well -- two products for its two chunks instead of three)
                f_exec = 32768.0 * (n_b * (5 * 4 * 2 + 2 * 4 * 2) + n_t * ((8 * 3 + 2 * 2 + 8 * 3) if use_pack else (10 + 8) * 3) * 4)
            else:
                f_exec = 2.0 * (2.0 * E * 72 * 128) + 3.0 * (2.0 * N * ((28 + 128 + 4) * 128 + 128 * 128))
            t_hbm, t_mfma = b_launch / (HBM_PEAK_GBS * 1e9), f_exec / (MFMA_BF16_PEAK_TF * 1e12)
            hbm = b_launch / t_k / 1e9
            executed = f_exec / t_k / 1e12
            common = {"kernel": (("layer_fused_kernel_rp<4,2> (csrc/layer_rp.hip, inputs as exact fp16 row packs: " if use_pack else "layer_fused_kernel_rr<4,2> (csrc/layer_rr.hip: ")
                                 if rr else "layer_fused_kernel<5,10,8,4> (csrc/layer_fused.hip: ") +
                                "edge stage + per-node sums + node stages 0 and 1 in one launch)",
                      "matrix_dtype": "fp16x3: operands split into two fp16 planes after exact power-of-two row / matrix scaling, three plane "
                                      "products per fp32 product on v_mfma_f32_32x32x16_f16 with fp32 accumulation (two where the rows are exact in fp16)",
                      "algorithmic_bytes": round(b_launch), "survey_B_alg_bytes": round(survey_b_alg),
                      "hbm_GBs": round(hbm, 1), "hbm_frac": round(hbm / HBM_PEAK_GBS, 4),
                      "survey_hbm_frac": round(survey_b_alg / t_k / (HBM_PEAK_GBS * 1e9), 4),
                      "mfma_executed_TFLOPs": round(executed, 1), "mfma_frac": round(executed / MFMA_BF16_PEAK_TF, 4),
                      "fp32_equivalent_TFLOPs": round(f_alg / t_k / 1e12, 2), "fp32_mfma_peak_TFLOPs": MFMA_F32_PEAK_TF,
                      "roof_ms_per_launch": {"hbm": round(t_hbm * 1e3, 4), "mfma_f16": round(t_mfma * 1e3, 4)}}
            if t_hbm >= t_mfma:
                roof = dict(common, bound="hbm", achieved=round(hbm, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(hbm / HBM_PEAK_GBS, 4), traffic=None)
            else:      # the executed plane products at the dense f16 MFMA peak take longer than the bytes at the HBM peak
                roof = dict(common, bound="mfma", achieved=round(executed, 1), peak=MFMA_BF16_PEAK_TF, unit="TFLOP/s",
                            frac=round(executed / MFMA_BF16_PEAK_TF, 4), traffic=None)
        elif dom in ("linear_fwd", "mlp_chain"):
            ach = kd["work_per_step"] / (kd["ms_per_step"] * 1e-3) / 1e12
            roof = {"kernel": {"linear_fwd": "linear_fwd_kernel", "mlp_chain": "mlp_chain1_seg_bf16_kernel + mlp_chain2_pipe_bf16_kernel (GSN_LAYER_FUSED=0)"}[dom],
                    "bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s (fp32-equivalent)",
                    "frac": round(ach / MFMA_F32_PEAK_TF, 4), "traffic": None,
                    "survey_hbm_frac": round(survey_b_alg / (kd["ms_per_step"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)}
        else:
            ach = kd["work_per_step"] / (kd["ms_per_step"] * 1e-3) / 1e9
            roof = {"kernel": {"propagate_fwd": "propagate_fwd_kernel", "count": "count_kernel"}[dom], "bound": "hbm",
                    "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None}
        # HBM traffic cannot be read from inside the run: PMC needs rocprofv3 around the process.  Report the committed
        # measurement of the same command (scripts/profile_bench.sh -> profiles/r04_bench_pmc.csv): per launch of the dominant
        # kernel, FETCH_SIZE x2 (gfx950 under-reports wide reads, MI355X_MICROARCH.md) + WRITE_SIZE, in bytes.
        try:
            import csv
            import glob
            pmc = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r[0-9][0-9]_bench_pmc.csv")))[-1]   # the latest round's
            pmc_name = "profiles/" + os.path.basename(pmc)
            key = {"layer_fused": "gsn::layer_fused_kernel", "mlp_chain": "gsn::mlp_chain"}.get(dom, roof["kernel"])   # (not layer_fused_prepare_kernel)
            rows = [r for r in csv.DictReader(open(pmc)) if key in r["kernel"]]
            if rows and G == 65536:
                tot = sum((2.0 * float(r["FETCH_SIZE_per_dispatch"]) + float(r["WRITE_SIZE_per_dispatch"])) * 1024.0 for r in rows)
                roof["traffic"] = round(tot / len(rows))
                roof["traffic_source"] = pmc_name + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command)"
            crow = [r for r in csv.DictReader(open(pmc)) if "count_kernel" in r["kernel"]]
            if crow and G == 65536:      # the counting kernel is VALU-bound, not bandwidth-bound -- show it
                r0 = crow[0]
                pmc_count = {"valu_busy_frac_of_wave_cycles": round(float(r0["SQ_ACTIVE_INST_ANY_per_dispatch"]) / float(r0["SQ_WAVE_CYCLES_per_dispatch"]), 4),
                             "valu_instructions_per_dispatch": float(r0["SQ_INSTS_VALU_per_dispatch"]),
                             "hbm_bytes_per_dispatch": round((2.0 * float(r0["FETCH_SIZE_per_dispatch"]) + float(r0["WRITE_SIZE_per_dispatch"])) * 1024.0),
                             "source": pmc_name}
            else:
                pmc_count = None
        except Exception:
            pmc_count = None
        roof["launches_per_step"] = kd["launches_per_step"]
        roof["avg_launch_ms"] = round(kd["ms_per_step"] / kd["launches_per_step"], 4)
        ck = kernels["count"]
        extra = {}
        if "propagate_fwd" in kernels:   # only when the scatter-add is not fused into the edge stage
            pk = kernels["propagate_fwd"]
            extra["propagate_hbm_GBs"] = round(pk["work_per_step"] / (pk["ms_per_step"] * 1e-3) / 1e9, 1)
            extra["propagate_hbm_frac"] = round(pk["work_per_step"] / (pk["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        extra.update({
            "count_graphs_per_s": round(G / (ck["ms_per_step"] * 1e-3), 1),
            # SURVEY 8(d) work figures, from the output alone: occurrence-positions = sum of all counts; maps = sum_p
            # aut_p * (pattern p's column sums) / (2 |E(H_p)|)
            "count_occurrence_positions_per_s": round(occ_pos / (ck["ms_per_step"] * 1e-3), 1),
            "count_maps_per_s": round(n_maps / (ck["ms_per_step"] * 1e-3), 1),
            "count_hbm_GBs": round(ck["work_per_step"] / (ck["ms_per_step"] * 1e-3) / 1e9, 1),
            "count_pmc": pmc_count,
            # SURVEY 8(d) for HP-1: integer vector work against the chip's integer-VALU ceiling (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz =
            # 78.6 T lane-ops/s) -- the counting kernel is neither bandwidth- nor issue-bound but latency-bound (profiles/r05_count_phase_profile.txt)
            "count_roofline": None if pmc_count is None else {
                "lane_ops_per_s": round(pmc_count["valu_instructions_per_dispatch"] * 64.0 / (ck["ms_per_step"] * 1e-3), 1),
                "frac_of_78.6T_integer_valu": round(pmc_count["valu_instructions_per_dispatch"] * 64.0 / (ck["ms_per_step"] * 1e-3) / 78.6e12, 4),
                "valu_busy": pmc_count["valu_busy_frac_of_wave_cycles"],
                "hbm_frac": round(ck["work_per_step"] / (ck["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "bound": "latency x occupancy (5 one-wave workgroups per SIMD): not VALU issue, not HBM",
                "valu_instructions_source": pmc_count["source"]},
            "ms_per_step_by_kernel": per_launch,
            "host_enqueue_ms_per_step": round(t_enq / args.steps * 1e3, 4),
            "eager_ms_per_step": round(dt_eager / args.steps * 1e3, 4),
            "hip_graph_ms_per_step": None if dt_graph is None else round(dt_graph / args.steps * 1e3, 4),
            # the eager steps timed beside the replays (alternately, behind the oracle checks): what hip_graph_ms_per_step compares with
            "eager_beside_hip_graph_ms_per_step": None if not res_eager_late else round(min(res_eager_late.values()) / args.steps * 1e3, 4),
            "hip_graph_forked_ms_per_step": None if dt_graph_fork is None else round(dt_graph_fork / args.steps * 1e3, 4),
            "step_prepacked": None if dt_pre is None else {
                "ms_per_step": round(dt_pre / args.steps * 1e3, 4), "graphs_per_s": round(world * G * args.steps / dt_pre, 1),
                "note": "the headline step of rounds 2-4: dense one-hot x / bond rows and their fp16 packs made outside the step, no int64 identifiers written"},
            "step_without_int64_ids": None if dt_noids is None else {
                "ms_per_step": round(dt_noids / args.steps * 1e3, 4), "graphs_per_s": round(world * G * args.steps / dt_noids, 1),
                "note": "the headline step with the counting kernel writing the encoded identifier rows only"},
            "step_six_launches": None if dt_six is None else {
                "ms_per_step": round(dt_six / args.steps * 1e3, 4), "graphs_per_s": round(world * G * args.steps / dt_six, 1),
                "host_enqueue_ms_per_step": round(t_enq_six / args.steps * 1e3, 4),
                "note": "the r05 headline: CSR build + two code encoders on a second stream under the counting kernel, then the layer (six launches, eager)"},
            "layer_alone_ms": layer_alone,
            "launch": ("eager: one host call per step (gsn_count_layer_step_hip), two kernel launches; `value` is this timing, hip_graph_ms_per_step the same two "
                       "launches replayed from a captured graph") if one_call else "eager (six launches, second stream)",
        })
        if graph_note:
            extra["hip_graph_note"] = graph_note
        if fused is not None:
            extra["fused_encoder_step"] = fused
        if zinc12k is not None:
            extra["zinc12k_step"] = zinc12k
        if small is not None:
            extra["small_batch"] = small
        if prop is not None:
            extra["propagate"] = prop
        if flt is not None:
            extra["layer_float_inputs"] = flt
        if wide is not None:
            extra["layer_wide_d128"] = wide
        if train4 is not None:
            extra["train_step_config4"] = train4
        if train_small is not None:
            extra["train_small_batch"] = train_small
        if lin300 is not None:
            extra["linear_f16x3_d300"] = lin300
        if er128 is not None:
            extra["count_er128_config5"] = er128
        extra["ms_per_step_by_rank"] = per_rank_ms
        extra["graphs_by_rank"] = graphs_by_rank
        if rccl is not None:
            extra["rccl"] = rccl
        extra["prewarm_steps_untimed"] = int(os.environ.get("GSN_BENCH_PREWARM", "60"))
        if model4 is not None:
            extra["full_model_step"] = model4
        res = dict(headline_line(world, G, N, E, args, dt), **{
            "roofline": roof, "kernels": extra,
            "counts_checked": bool(checked["counts_bit_exact"]), "checked": checked,
            "tolerance": "counts bit-exact (int64); layer output vs the fp32 oracle: |got-ref| <= 1e-5 |ref| + 1e-5 max|ref row| element-wise",
        })
        assert checked["counts_bit_exact"], "timed counts differ from the oracle"
        assert checked["layer_elementwise_1e-5_rel_plus_1e-5_rowmax"], "timed layer output differs from the oracle: %r" % (checked,)
        if not args.no_cpu_baseline and world == 1:
            res["cpu_baseline"] = cpu_baseline(seed=1000)
        print(json.dumps(res))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
