"""Training epochs over padded batches against eager epochs over the unpadded DataLoader, by 8c's protocol: ONE process, both
variants warmed up, then alternated; the median of ``--epochs`` epochs with min .. max; host clock, every measurement ends in a synchronise.

    (a) eager      steps over gsn_amd.loader.DataLoader: collate launch, forward, masked loss, backward, gsn_amd.optim.Adam -- the path a real
                   epoch (a different vertex and edge count in every batch) had before
    (b) padded     graphs.PaddedTrainStep over gsn_amd.loader.PaddedDataLoader: collate launch + ONE graph replay per batch

on 8e's two shapes: the molhiv-shaped GNN_OGB (5 x 300, virtual node) at B = 32 and the ZINC-shaped GNNSubstructures (4 x 128) at B = 128.
Then gsn_bn_finalize_bounded_hip alone against gsn_bn_finalize_count_hip at [N_cap, 300] with 50 % and 90 % of the rows real.

    python scripts/bench_padded_train.py [--epochs 7] [--graphs 512] [--out profiles/padded_train_bench.jsonl]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
import types

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
from gsn_amd import _abi  # noqa: E402
from gsn_amd import evaluation as ev  # noqa: E402
from gsn_amd.graphs import PaddedTrainStep  # noqa: E402
from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader  # noqa: E402
from gsn_amd.optim import Adam  # noqa: E402


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def molhiv_case(n_graphs, batch, dev):
    """(model, graphs, loss kind): scripts/train_step_molhiv.py's model and its evaluation set's graphs (random codes, 20 % NaN labels)"""
    m = _script("train_step_molhiv")
    model, _, _, _, _, _, _ = m.build(types.SimpleNamespace(batch=batch, layers=5, d=300, optimizer="sgd"), dev, 0)
    graphs = m.dataset_graphs(n_graphs, model.identifier_dims, 900)
    return model, graphs, "BCEWithLogitsLoss"


def zinc_case(n_graphs, batch, dev):
    """(model, graphs, loss kind): scripts/train_step_zinc.py's model over its --loader dataset"""
    import networkx as nx
    from gsn_amd.counting import CountPlan
    m = _script("train_step_zinc")
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    loader, d_id = m.native_loader(types.SimpleNamespace(loader_graphs=n_graphs, batch=batch), dev, 0, plan)
    model, _, _ = m.make_model(types.SimpleNamespace(optimizer="sgd"), dev, d_id)
    return model, loader.dataset, "L1Loss"


def bench_epochs(name, model, graphs, kind, batch, epochs, dev):
    ds = graphs if isinstance(graphs, DeviceDataset) else DeviceDataset(graphs, device=dev)
    plain, padded = DataLoader(ds, batch_size=batch), PaddedDataLoader(ds, batch_size=batch)
    model.train()
    opt = Adam(model.parameters(), lr=1e-4)
    params = list(model.parameters())

    def eager_epoch():
        for data in plain:
            opt.zero_grad(set_to_none=True)
            ev.masked_loss(kind, model(data), data.y).backward()
            opt.step()

    step = PaddedTrainStep(model, padded, kind, opt, params)
    variants = {"eager": eager_epoch, "padded": step.run_epoch}
    for fn in variants.values():          # warm-up: allocator, caches, the capture
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in variants}
    for _ in range(epochs):
        for k, fn in variants.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[k].append((time.perf_counter() - t0) / len(plain) * 1e3)
    assert step.captures == 1 and step.eager_batches == 0
    out = []
    for k, ts in times.items():
        out.append({"bench": "padded_train_epoch", "shape": name, "variant": k, "batch": batch, "graphs": len(ds), "batches": len(plain),
                    "epochs": epochs, "ms_per_batch_median": round(statistics.median(ts), 4), "ms_per_batch_min": round(min(ts), 4),
                    "ms_per_batch_max": round(max(ts), 4), "node_capacity": padded.node_capacity, "edge_capacity": padded.edge_capacity,
                    "graph_slots": padded.graph_slots})
    return out, padded.node_capacity


def bench_finalize(n_cap, c, dev, reps=200):
    """gsn_bn_finalize_bounded_hip against gsn_bn_finalize_count_hip at [n_cap, c], device time per launch (events around ``reps`` launches)"""
    L = _abi.lib()
    h = torch.randn(n_cap, c, device=dev)
    stats = torch.stack([h.double().sum(0), (h.double() ** 2).sum(0)]).contiguous()
    vec = torch.empty(4, c, device=dev)
    p0 = vec.data_ptr()
    words = int(L.gsn_bn_finalize_bounded_scratch_bytes(c)) // 8
    scratch = torch.zeros(reps, words, dtype=torch.float64, device=dev)
    n_valid = torch.zeros(1, dtype=torch.int64, device=dev)
    s = _abi.current_stream()
    out = []

    def timed(fn):
        for i in range(10):
            fn(i)
        scratch.zero_()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps * 1e3

    count = lambda i: _abi.check(L.gsn_bn_finalize_count_hip(c, n_cap, 1e-5, 0.0, stats.data_ptr(), None, None, None, None, p0, p0 + 4 * c, p0 + 8 * c,
                                                            p0 + 12 * c, None, s), "count")
    bounded = lambda i: _abi.check(L.gsn_bn_finalize_bounded_hip(c, n_cap, 1e-5, 0.0, stats.data_ptr(), h.data_ptr(), n_valid.data_ptr(), None, 0,
                                                                 scratch[i].data_ptr(), None, None, None, None, p0, p0 + 4 * c, p0 + 8 * c, p0 + 12 * c,
                                                                 None, s), "bounded")
    base = [timed(count) for _ in range(3)]
    # what a bounded stage of at most flags.FUSE_BN_ACT_ROWS rows pays for not fusing the activation pass: finalize + gsn_bn_act_hip as two
    # launches (bounded) against gsn_bn_finalize_act_hip's one (unbounded stages of that size)
    y = torch.empty_like(h)

    def act_pass():
        _abi.check(L.gsn_bn_act_hip(n_cap, c, h.data_ptr(), p0, p0 + 8 * c, p0 + 12 * c, 1, y.data_ptr(), s), "bn_act")

    def fused(i):
        _abi.check(L.gsn_bn_finalize_act_hip(c, n_cap, 1e-5, 0.0, stats.data_ptr(), None, None, None, None, p0, p0 + 4 * c, p0 + 8 * c, p0 + 12 * c, None,
                                             h.data_ptr(), 1, y.data_ptr(), s), "finalize_act")

    def bounded_then_act(i):
        bounded(i)
        act_pass()

    n_valid.fill_(int(n_cap * 0.9))
    t_fused, t_two = [timed(fused) for _ in range(3)], [timed(bounded_then_act) for _ in range(3)]
    out.append({"bench": "bn_finalize_act_unfused", "rows": n_cap, "cols": c, "real_share": 0.9, "us_finalize_act_one_launch": round(statistics.median(t_fused), 3),
                "us_bounded_then_bn_act": round(statistics.median(t_two), 3)})
    for share in (0.5, 0.9):
        n_valid.fill_(int(n_cap * share))
        ts = []
        for _ in range(3):
            ts.append(timed(bounded))
        out.append({"bench": "bn_finalize_bounded", "rows": n_cap, "cols": c, "real_share": share, "us_bounded_median": round(statistics.median(ts), 3),
                    "us_count_median": round(statistics.median(base), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "padded_train_bench.jsonl"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []
    model, graphs, kind = molhiv_case(args.graphs, 32, dev)
    res, n_cap = bench_epochs("molhiv-shaped GNN_OGB 5 x 300 vn", model, graphs, kind, 32, args.epochs, dev)
    lines += res
    model, graphs, kind = zinc_case(args.graphs, 128, dev)
    res, _ = bench_epochs("ZINC-shaped GNNSubstructures 4 x 128", model, graphs, kind, 128, args.epochs, dev)
    lines += res
    lines += bench_finalize(n_cap, 300, dev)
    with open(args.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
