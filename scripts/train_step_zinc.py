#!/usr/bin/env python3
"""BASELINE configs[1] as a TRAINING step (README.md:112 flags): GNNSubstructures, GSN_edge_sparse general, 4 layers, d=128,
one-hot atom / bond / identifier encoders, cycle counts k<=6 (GSN-e, local), sum readout, L1 loss, batch 128 per GPU; graph-shard
data parallel with one flat RCCL gradient all-reduce per step.  Forward and backward run on the HIP kernels.

    python scripts/train_step_zinc.py [--batch 128] [--steps 20]
    python scripts/train_step_zinc.py --loader native          # eager steps over batches of a device-resident DataLoader (gsn_amd.loader)
    python scripts/train_step_zinc.py --loader padded          # the same batches padded to one shape: collate launch + ONE graph replay per step
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 scripts/train_step_zinc.py"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import networkx as nx

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gsn_amd import dist as gdist, encoding, models, synth  # noqa: E402
from gsn_amd.counting import CountPlan, count_batch  # noqa: E402


def native_loader(args, dev, rank, plan, padded=False):
    """``--loader native``: a prepared ZINC-shaped dataset of ``--loader-graphs`` graphs on the device and a shuffled DataLoader over it
    (gsn_amd.loader: one HIP launch per batch); ``padded``: a PaddedDataLoader, every batch in one set of static tensors.  -> (loader, d_id)"""
    from gsn_amd.data import Data
    from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader
    b = synth.zinc_shape_batch(max(args.loader_graphs, args.batch), seed=200 + rank)
    ids, _ = count_batch(plan, b.node_ptr, b.edge_ptr, torch.from_numpy(b.edge_index), ids_are_global=True, device=dev)
    codes, d_id = encoding.unique_codes(ids)
    codes = codes.cpu()
    rng = np.random.default_rng(rank)
    graphs = []
    for g in range(b.num_graphs):
        n0, n1, e0, e1 = int(b.node_ptr[g]), int(b.node_ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        graphs.append(Data(edge_index=torch.from_numpy(b.edge_index[:, e0:e1] - n0), x=torch.from_numpy(b.atom_type[n0:n1]).unsqueeze(1),
                           graph_size=n1 - n0, degrees=torch.zeros(n1 - n0), edge_features=torch.from_numpy(b.bond_type[e0:e1]).unsqueeze(1),
                           y=torch.from_numpy(rng.standard_normal(1).astype(np.float32)), identifiers=codes[e0:e1].clone()))
    gen = torch.Generator()
    gen.manual_seed(rank)
    cls = PaddedDataLoader if padded else DataLoader
    return cls(DeviceDataset(graphs, device=dev), batch_size=args.batch, shuffle=True, drop_last=True, generator=gen), d_id


def build(args, dev, rank=0):
    """(model, data, params, optimizer, loss closure, N, E) of the step."""
    if getattr(args, "loader", "static") == "native":
        return build_native(args, dev, rank)
    if getattr(args, "loader", "static") == "padded":
        return build_padded(args, dev, rank)
    b = synth.zinc_shape_batch(args.batch, seed=200 + rank)
    N, E = b.num_nodes, b.num_edges
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    ids, _ = count_batch(plan, b.node_ptr, b.edge_ptr, torch.from_numpy(b.edge_index), ids_are_global=True, device=dev)
    codes, d_id = encoding.unique_codes(ids)
    rng = np.random.default_rng(rank)
    data = types.SimpleNamespace(x=torch.from_numpy(b.atom_type).unsqueeze(1).to(dev), edge_index=torch.from_numpy(b.edge_index).to(dev),
                                 edge_features=torch.from_numpy(b.bond_type).unsqueeze(1).to(dev), identifiers=codes.to(dev),
                                 batch=torch.from_numpy(np.asarray(b.batch).astype(np.int64)).to(dev), degrees=torch.zeros(N, device=dev),
                                 y=torch.from_numpy(rng.standard_normal((args.batch, 1)).astype(np.float32)).to(dev))
    if os.environ.get("GSN_TRAIN_PARTITION", "1") != "0":
        # the collated batch's graph boundaries (what the counting kernel takes as well): the layers' aggregation index is then ONE launch per
        # direction (gsn_csr_build_graphs_hip) instead of the generic build, the readout needs none (models._register_partition)
        data.graph_partition = (torch.from_numpy(b.node_ptr.astype(np.int64)).to(dev), torch.from_numpy(b.edge_ptr.astype(np.int64)).to(dev),
                                int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max()), False)
    model, params, opt = make_model(args, dev, d_id)
    loss_fn = torch.nn.L1Loss()
    return model, data, params, opt, (lambda: loss_fn(model(data), data.y)), N, E


def build_native(args, dev, rank):
    """The same model stepping over the batches of a DataLoader: every step draws the next batch (a new epoch when one runs out)."""
    if getattr(args, "graph", False):
        raise SystemExit("--loader native draws batches of varying shapes: they cannot be replayed as one HIP graph (drop --graph)")
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    loader, d_id = native_loader(args, dev, rank, plan)
    model, params, opt = make_model(args, dev, d_id)
    loss_fn = torch.nn.L1Loss()
    state = {"it": iter(loader)}

    def loss_of():
        batch = next(state["it"], None)
        if batch is None:
            state["it"] = iter(loader)
            batch = next(state["it"])
        return loss_fn(model(batch), batch.y.view(-1, 1))

    sizes = loader.dataset.host_sizes
    per_batch = args.batch / max(len(loader.dataset), 1)
    return model, None, params, opt, loss_of, int(sizes("x").sum() * per_batch), int(sizes("edge_index").sum() * per_batch)


def build_padded(args, dev, rank):
    """``--loader padded``: the batches of ``--loader native`` padded to one shape (gsn_amd.loader.PaddedDataLoader) and the whole step --
    forward under loader.masked_training, counted loss, backward, all-reduce, optimizer -- replayed as ONE HIP graph per batch
    (gsn_amd.graphs.PaddedTrainStep).  The "loss closure" returned here IS the step: run() calls nothing around it."""
    from gsn_amd.graphs import PaddedTrainStep
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    loader, d_id = native_loader(args, dev, rank, plan, padded=True)
    model, params, opt = make_model(args, dev, d_id)
    padded_step = PaddedTrainStep(model, loader, "L1Loss", opt, params, warmup=max(1, getattr(args, "warmup", 1)))
    state = {"it": iter(loader)}

    def step():
        batch = next(state["it"], None)
        if batch is None:
            state["it"] = iter(loader)
            batch = next(state["it"])
        return padded_step.step(batch)

    sizes = loader.dataset.host_sizes
    per_batch = args.batch / max(len(loader.dataset), 1)
    return model, None, params, opt, step, int(sizes("x").sum() * per_batch), int(sizes("edge_index").sum() * per_batch)


def make_model(args, dev, d_id):
    L, d = 4, 128
    act = getattr(args, "activation", "relu")      # (the tests of replay == eager use elu: no ReLU kink for last-bit noise to flip)
    p_drop = float(getattr(args, "dropout_p", 0.0))      # (README.md:112 trains without dropout)
    kw = dict(seed=0, model_name="GSN_edge_sparse", readout="sum", dropout_features=[p_drop] * (L + 1), bn=[True] * L,
              dropout_impl=getattr(args, "dropout", None),
              final_projection=list(getattr(args, "final_projection", None) or [False] * L + [True]), inject_ids=False, inject_edge_features=True, random_features=False,
              id_scope="local", d_msg=[d] * L, d_out=[d] * L, d_h=[[d]] * L, aggr="add", flow="source_to_target",
              msg_kind="general", train_eps=[False] * L, activation_mlp=act, bn_mlp=True, jk_mlp=True, degree_embedding="None",
              degree_as_tag=[False] * L, retain_features=[True] * L, multi_embedding_aggr="sum", input_node_encoder="one_hot_encoder",
              d_out_node_encoder=d, edge_encoder="one_hot_encoder", d_out_edge_encoder=[d] * L, id_embedding="one_hot_encoder",
              d_out_id_embedding=d, d_out_degree_embedding=d, extend_dims=True, activation=act)
    torch.manual_seed(0)
    model = models.GNNSubstructures(1, 1, None, d_id, 1, [28], [4], None, None, **kw).to(dev).train()
    params = list(model.parameters())
    if getattr(args, "optimizer", "sgd") == "adam":
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
    elif getattr(args, "optimizer", "sgd") == "adam_native":
        from gsn_amd import optim
        opt = optim.Adam(params, lr=1e-3)          # one HIP launch per step; a replay follows the schedulers (gsn_amd/optim.py)
    else:
        opt = torch.optim.SGD(params, lr=1e-3)
    return model, params, opt


def run(args, dev, dist=None, rank=0, world=1):
    """The timed steps; the result line as a dict (bench.py `train_small_batch` calls this)."""
    model, data, params, opt, loss_of, N, E = build(args, dev, rank)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_of()
        loss.backward()
        gdist.allreduce_gradients(params, average=True)
        opt.step()
        return loss

    padded = getattr(args, "loader", "static") == "padded"
    if padded:
        step = loss_of          # (build_padded: the replayed step itself)
    elif getattr(args, "graph", False):
        from gsn_amd.graphs import GraphedTrainStep
        step = GraphedTrainStep(loss_of, opt, params, warmup=max(1, args.warmup))
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    n_params = sum(p.numel() for p in params)
    res = ({"workload": "ZINC-shaped GNNSubstructures training step (4 x GSN_edge_sparse general d=128), batch %d graphs/GPU (N=%d, E=%d)" % (args.batch, N, E),
            "n_gpus": world, "graphs_per_s": round(world * args.batch * args.steps / dt, 1),
            "ms_per_step": round(dt / args.steps * 1e3, 3), "parameters": n_params, "loss": float(loss.item()),
            "launch": "hip_graph" if (getattr(args, "graph", False) or padded) else "eager", "optimizer": getattr(args, "optimizer", "sgd")})
    if getattr(args, "loader", "static") != "static":
        res["loader"] = args.loader          # (N, E of the workload line: the dataset's mean per batch)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graph", action="store_true", help="replay the whole step as one HIP graph (gsn_amd.graphs.GraphedTrainStep)")
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "adam", "adam_native"])
    ap.add_argument("--loader", default="static", choices=["static", "native", "padded"],
                    help="static: one batch built by hand, every step on it; native: batches of a device-resident gsn_amd.loader.DataLoader; "
                         "padded: the same batches in the static tensors of a PaddedDataLoader, the step replayed as one HIP graph per batch")
    ap.add_argument("--loader-graphs", type=int, default=1024, help="graphs of the dataset behind --loader native / padded")
    ap.add_argument("--dropout", default=None, choices=["torch", "native"],
                    help="native: gsn_amd.dropout on the jumping-knowledge projections (default: GSN_DROPOUT, else torch)")
    ap.add_argument("--dropout-p", type=float, default=0.0, help="dropout probability of the projections (the reference's run uses none)")
    args = ap.parse_args()
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if "RANK" in os.environ:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    res = run(args, dev, dist, rank, world)
    if rank == 0:
        print(json.dumps(res))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
