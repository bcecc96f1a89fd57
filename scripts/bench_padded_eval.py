#!/usr/bin/env python3
"""An evaluation epoch over the device-resident loaders, eager against replayed:

  eager          evaluation.test_ogb / test over gsn_amd.loader.DataLoader: per batch one collate launch, the eager eval forward (Python in
                 front of ~100 small launches) and one accumulate call -- the baseline
  padded         the same call over gsn_amd.loader.PaddedDataLoader with default capacities: per batch one padded collate launch and ONE
                 replay of the HIP graph that evaluation.GraphedEpoch captured (forward + counted accumulation)
  padded_p99     the same with capacities set to the 99th-percentile batch: less padding, the few larger batches run eagerly

Configurations: the molhiv-shaped GNN_OGB (5 x 300, virtual node; 20 % NaN labels; ROC-AUC) at B = 32 and 128, and the ZINC-shaped
GNNSubstructures of scripts/train_step_zinc.py at B = 128 (L1 loss and L1 sum).  One process; every variant is warmed up with one epoch,
then the variants are run alternately; median of --repeats epochs with min - max, a host clock around the epoch ending in a synchronise.
Also reported: the padding ratio N_cap / mean N_r, the kernels of one captured step (counted on an eager run of the captured function under
torch.profiler, None where the profiler gives no device events) and the share of them that remakes derived weights (the difference to a run
that finds the caches warm).

    python scripts/bench_padded_eval.py [--out profiles/padded_eval_bench.jsonl] [--repeats 7] [--molhiv-batches 300] [--zinc-batches 94]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from gsn_amd import encoding, evaluation as ev, layers, models, synth  # noqa: E402
from gsn_amd.data import Data  # noqa: E402
from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader, padded_shape  # noqa: E402


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def molhiv_setup(n_graphs, dev, layers_=5, d=300, nan_share=0.2):
    """molhiv-shaped prepared graphs (random codes within ogb's feature dims, four identifier columns of three codes) and the model of
    scripts/train_step_molhiv.py in eval mode"""
    b = synth.zinc_shape_batch(n_graphs, seed=0, mean_n=25.5, sd_n=8.0, n_min=4, n_max=60)
    rng = np.random.default_rng(0)
    x = np.stack([rng.integers(0, k, b.num_nodes) for k in encoding.ATOM_FEATURE_DIMS], 1)
    ef = np.stack([rng.integers(0, k, b.num_edges) for k in encoding.BOND_FEATURE_DIMS], 1)
    ids = rng.integers(0, 3, (b.num_edges, 4))
    y = rng.integers(0, 2, (n_graphs, 1, 1)).astype(np.float32)
    y[rng.random((n_graphs, 1, 1)) < nan_share] = np.nan
    graphs = []
    for g in range(n_graphs):
        n0, n1, e0, e1 = int(b.node_ptr[g]), int(b.node_ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        graphs.append(Data(edge_index=torch.from_numpy(b.edge_index[:, e0:e1] - n0), x=torch.from_numpy(x[n0:n1]), degrees=torch.zeros(n1 - n0),
                           edge_features=torch.from_numpy(ef[e0:e1]), y=torch.from_numpy(y[g]), identifiers=torch.from_numpy(ids[e0:e1])))
    L = layers_
    kw = dict(seed=0, model_name="GSN_edge_sparse_ogb", readout="mean", dropout_features=[0.5] * (L + 1), bn=[True] * L,
              final_projection=[False] * L + [True], residual=False, inject_ids=True, vn=True, id_scope="local",
              d_msg=[d] * L, d_out=[d] * L, d_h=[[2 * d]] * L, aggr="add", flow="source_to_target", msg_kind="ogb",
              train_eps=[True] * L, activation_mlp="relu", bn_mlp=True, jk_mlp=False, degree_embedding="None",
              degree_as_tag=[False] * L, retain_features=[True] * L, multi_embedding_aggr="sum", features_scope="full",
              input_node_encoder="atom_encoder", d_out_node_encoder=d, input_vn_encoder="embedding", d_out_vn_encoder=d,
              edge_encoder="bond_encoder", d_out_edge_encoder=[d] * L, id_embedding="embedding", d_out_id_embedding=d,
              d_out_degree_embedding=d, d_out_vn=[d] * (L - 1), vn_pooling="sum", extend_dims=True, activation="relu")
    torch.manual_seed(0)
    model = models.GNN_OGB(9, 1, None, [3, 3, 3, 3], 3, None, None, None, None, **kw).to(dev).eval()
    evaluator = ev.Evaluator("ogbg-molhiv")
    loss = ev.MaskedLoss("BCEWithLogitsLoss")
    return graphs, model, (lambda loader: ev.test_ogb(loader, model, loss, dev, evaluator)), "GNN_OGB 5 x 300 + vn, molhiv-shaped, 20 % NaN labels"


def zinc_setup(n_graphs, dev):
    import types
    ts = _script("train_step_zinc")
    from gsn_amd.counting import CountPlan
    import networkx as nx
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    args = types.SimpleNamespace(loader_graphs=n_graphs, batch=1)
    loader, d_id = ts.native_loader(args, dev, 0, plan)
    model, _, _ = ts.make_model(types.SimpleNamespace(), dev, d_id)
    model.eval()
    return loader.dataset, model, (lambda ld: ev.test(ld, model, "L1Loss", dev, prediction_fn="L1Loss")), "GNNSubstructures 4 x 128 (train_step_zinc), ZINC-shaped"


def p99_capacities(n, e, B):
    """capacities that hold the 99th-percentile batch of the sequential loader: E_cap = p99(E_r), N_cap = p99(N_r) + the pad slots it implies"""
    starts = np.arange(0, len(n), B)
    n_r, e_r = np.add.reduceat(n, starts), np.add.reduceat(e, starts)
    e_cap = int(np.percentile(e_r, 99))
    n99 = int(np.percentile(n_r, 99))
    n_cap = n99 + 1
    for _ in range(8):
        sh = padded_shape(n, e, B, node_capacity=n_cap, edge_capacity=e_cap)
        n_cap = n99 + sh.pad_slots
    return n_cap, e_cap


def count_kernels(fn):
    """device kernels of one call of fn, or None where the profiler gives none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return n or None
    except Exception:
        return None


def bench_config(name, graphs, model, run, what, B, args, dev):
    ds = graphs if isinstance(graphs, DeviceDataset) else DeviceDataset(graphs, device=dev)
    n, e = ds.host_sizes("x"), ds.host_sizes("edge_index")
    n_cap99, e_cap99 = p99_capacities(n, e, B)
    loaders = {"eager": DataLoader(ds, batch_size=B), "padded": PaddedDataLoader(ds, batch_size=B),
               "padded_p99": PaddedDataLoader(ds, batch_size=B, node_capacity=n_cap99, edge_capacity=e_cap99)}
    n_batches = len(loaders["eager"])
    results = {}
    for k, ld in loaders.items():                                  # warm-up: kernel loads, allocator pools, the capture
        results[k] = run(ld)
    torch.cuda.synchronize()
    ms = {k: [] for k in loaders}
    for _ in range(args.repeats):
        for k, ld in loaders.items():                              # alternately, in one process
            t0 = time.perf_counter()
            results[k] = run(ld)
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
    mean_n = float(np.add.reduceat(n, np.arange(0, len(n), B)).mean())
    line = {"bench": "padded_eval_epoch", "config": name, "model": what, "batch_size": B, "batches": n_batches, "graphs": len(ds), "repeats": args.repeats,
            "device": torch.cuda.get_device_name(dev), "arch": torch.cuda.get_device_properties(dev).gcnArchName,
            "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "mean_real_nodes_per_batch": round(mean_n, 1)}
    for k, ld in loaders.items():
        v = sorted(ms[k])
        line[k] = {"epoch_ms_median": statistics.median(v), "epoch_ms_min": v[0], "epoch_ms_max": v[-1],
                   "ms_per_batch": round(statistics.median(v) / n_batches, 4), "loss": results[k][0], "metric": results[k][1]}
        if k != "eager":
            (epoch,) = ld.graphed_epochs.values()
            line[k].update(node_capacity=ld.node_capacity, edge_capacity=ld.edge_capacity, graph_slots=ld.graph_slots,
                           padding_ratio=round(ld.node_capacity / mean_n, 3), captures=epoch.captures,
                           eager_batches_per_epoch=sum(1 for bt in ld if not getattr(bt, "padded", False)),
                           loss_difference=abs(results[k][0] - results["eager"][0]), metric_difference=abs(results[k][1] - results["eager"][1]))
    # the launches of one captured step, and how many of them remake what the caches would hold
    ld = loaders["padded"]
    (epoch,) = ld.graphed_epochs.values()
    batch = next(iter(ld))
    with torch.no_grad():
        def warm():
            pred = model(batch)
            epoch.acc.add(pred, epoch._target(batch, pred), n_valid=batch.n_valid)
        warm()
        cold_n = count_kernels(lambda: epoch._forward(batch))
        warm()
        warm_n = count_kernels(warm)
    layers.invalidate_caches(model)
    line["kernels_per_replay"] = cold_n
    line["kernels_with_warm_caches"] = warm_n
    line["derived_weight_share"] = round((cold_n - warm_n) / cold_n, 3) if cold_n and warm_n else None
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--molhiv-batches", type=int, default=300)
    ap.add_argument("--zinc-batches", type=int, default=94)
    ap.add_argument("--configs", nargs="+", default=["molhiv32", "molhiv128", "zinc128"], choices=["molhiv32", "molhiv128", "zinc128"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    for cfg in args.configs:
        B = 32 if cfg.endswith("32") else 128
        if cfg.startswith("molhiv"):
            graphs, model, run, what = molhiv_setup(B * args.molhiv_batches, dev)
        else:
            graphs, model, run, what = zinc_setup(B * args.zinc_batches, dev)
        lines.append(bench_config(cfg, graphs, model, run, what, B, args, dev))
        del graphs, model, run
        layers.drop_input_caches()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
