#!/usr/bin/env python3
"""One epoch of collated batches, three ways, on ZINC-shaped (~12 k graphs) and molhiv-shaped (~41 k graphs) prepared datasets at
B = 32, 128, 1 024, 4 096:

  (a) native        gsn_amd.loader.DataLoader: the dataset on the device, one HIP launch per batch (csrc/loader.hip)
  (b) host_collate  what torch_geometric's collate does on the host Data list -- per attribute torch.cat, edge_index raised by the running
                    vertex count, batch vector -- followed by .to(device) of every tensor
  (c) torch_gather  the same device-resident tensors as (a), gathered with torch ops: a row index per pointer class from
                    repeat_interleave / arange (output sizes known on the host: no synchronisation), index_select per field

Each is a host clock around the shuffled epoch ending in a synchronise, warmed up once, then repeated alternately (a, b, c, a, b, c, ..)
in this process.  Attribute VALUES are random (the loader moves bytes); shapes, dtypes and row counts are those of prepared datasets
(edge-mode identifiers of four columns).

    python scripts/bench_loader.py [--repeats 3] [--out profiles/loader_bench.jsonl]
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -o loader -- python scripts/bench_loader.py --trace-epochs 2
    python scripts/bench_loader.py --summarise DIR [--stats-out profiles/loader_kernel_stats.csv]      # the launches / copies of that run
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gsn_amd import synth  # noqa: E402
from gsn_amd.data import Data  # noqa: E402

SHAPES = {
    # name: (graphs, generator arguments, x columns, edge feature columns, y shape)
    "zinc": (12000, {}, 1, 1, (1,)),
    "molhiv": (41127, dict(mean_n=25.5, sd_n=12.0, n_min=2, n_max=222, ring_rate=2.0), 9, 3, (1, 1)),
}


def make_graphs(name, n_graphs=None, seed=0):
    """Prepared-dataset-shaped Data list (prepare_graphs' attribute order), random values."""
    G, kw, dx, de, yshape = SHAPES[name]
    G = n_graphs or G
    b = synth.zinc_shape_batch(G, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 28, (b.num_nodes, dx))
    ef = rng.integers(0, 4, (b.num_edges, de))
    ids = rng.integers(0, 3, (b.num_edges, 4))
    y = rng.standard_normal((G,) + yshape).astype(np.float32)
    graphs = []
    t = torch.from_numpy
    for g in range(G):
        n0, n1, e0, e1 = int(b.node_ptr[g]), int(b.node_ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        d = Data()
        d.edge_index = t(b.edge_index[:, e0:e1] - n0)
        d.x = t(x[n0:n1])
        d.graph_size = n1 - n0
        d.degrees = torch.zeros(n1 - n0)
        d.edge_features = t(ef[e0:e1])
        d.y = t(y[g])
        d.identifiers = t(ids[e0:e1])
        graphs.append(d)
    return graphs


def epoch_native(loader):
    n = 0
    for batch in loader:
        n += 1
    torch.cuda.synchronize()
    return n


def epoch_host_collate(graphs, perm, bs, dev):
    n = 0
    for lo in range(0, len(perm), bs):
        chosen = [graphs[i] for i in perm[lo:lo + bs]]
        out = Data()
        sizes = torch.tensor([g.x.shape[0] for g in chosen], dtype=torch.int64)
        ptr = torch.zeros(len(chosen) + 1, dtype=torch.int64)
        torch.cumsum(sizes, 0, out=ptr[1:])
        for name, v0 in chosen[0]:
            if isinstance(v0, (int, float)):
                t = torch.tensor([getattr(g, name) for g in chosen])
            elif name == "edge_index":
                t = torch.cat([g.edge_index + int(ptr[j]) for j, g in enumerate(chosen)], dim=1)
            else:
                t = torch.cat([getattr(g, name) for g in chosen], dim=0)
            setattr(out, name, t)
        out.batch = torch.repeat_interleave(torch.arange(len(chosen)), sizes)
        out.ptr = ptr
        out.to(dev)
        n += 1
    torch.cuda.synchronize()
    return n


class TorchGather:
    """(c): the DeviceDataset's own tensors and host sizes, batches gathered by torch ops."""

    def __init__(self, ds):
        self.ds, self.st = ds, ds._st
        self.rp_dev = torch.from_numpy(self.st.row_ptr).to(self.st.device)

    def epoch(self, perm, bs):
        st = self.st
        dev = st.device
        ids = self.ds._index[perm]
        sizes = st.sizes[:, ids]                                         # host [C, P]
        staged = torch.from_numpy(np.concatenate([ids[None, :], sizes], axis=0)).pin_memory()
        table = staged.to(dev, non_blocking=True)                        # one upload per epoch, as (a)
        ids_dev, sizes_dev = table[0], table[1:]
        n = 0
        for lo in range(0, len(ids), bs):
            hi = min(lo + bs, len(ids))
            g = ids_dev[lo:hi]
            index, excl = {}, {}
            for c in {f.cls for f in st.fields}:
                total = int(sizes[c, lo:hi].sum())
                cnt = sizes_dev[c, lo:hi]
                ex = torch.cumsum(cnt, 0) - cnt
                start = self.rp_dev[c].index_select(0, g) - ex
                index[c] = torch.repeat_interleave(start, cnt, output_size=total) + torch.arange(total, device=dev)
                excl[c] = ex
            out = Data()
            n_b = int(sizes[st.node_cls, lo:hi].sum())
            for f in st.fields:
                if f.name == "edge_index":
                    inc = torch.repeat_interleave(excl[st.node_cls], sizes_dev[f.cls, lo:hi], output_size=int(sizes[f.cls, lo:hi].sum()))
                    t = f.storage.index_select(1, index[f.cls]) + inc
                else:
                    t = f.storage.index_select(0, index[f.cls])
                setattr(out, f.name, t)
            out.batch = torch.repeat_interleave(torch.arange(hi - lo, device=dev), sizes_dev[st.node_cls, lo:hi], output_size=n_b)
            out.ptr = torch.cat([excl[st.node_cls], excl[st.node_cls][-1:] + sizes_dev[st.node_cls, hi - 1:hi]])
            n += 1
        torch.cuda.synchronize()
        return n


def timed(fn):
    t0 = time.perf_counter()
    n = fn()
    return (time.perf_counter() - t0) * 1e3, n


def bench(args):
    from gsn_amd.loader import DataLoader, DeviceDataset
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lines = []
    for name in args.datasets:
        graphs = make_graphs(name, args.graphs)
        ds = DeviceDataset(graphs, device=dev)
        gather = TorchGather(ds)
        for bs in args.batch_sizes:
            gen = torch.Generator()
            gen.manual_seed(bs)
            loader = DataLoader(ds, batch_size=bs, shuffle=True, generator=gen)
            perm_of = lambda: torch.randperm(len(graphs), generator=gen).numpy()
            runs = {"native": lambda: epoch_native(loader), "host_collate": lambda: epoch_host_collate(graphs, perm_of().tolist(), bs, dev),
                    "torch_gather": lambda: gather.epoch(perm_of(), bs)}
            for fn in runs.values():                                     # warm-up: allocator pools, kernel loads
                fn()
            ms = {k: [] for k in runs}
            n_batches = len(loader)
            for _ in range(args.repeats):
                for k, fn in runs.items():                               # alternately, in one process
                    t, n = timed(fn)
                    assert n == n_batches, (k, n, n_batches)
                    ms[k].append(round(t, 3))
            line = {"bench": "loader_epoch", "dataset": name, "graphs": len(graphs), "batch_size": bs, "batches": n_batches, "repeats": args.repeats}
            for k, v in ms.items():
                line[k + "_epoch_ms"] = v
                line[k + "_us_per_batch_median"] = round(statistics.median(v) * 1e3 / n_batches, 2)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


def trace_epochs(args):
    """(a) alone, for a kernel / memory-copy trace: `--trace-epochs` shuffled epochs of the ZINC-shaped dataset at B = 128."""
    from gsn_amd.loader import DataLoader, DeviceDataset
    torch.cuda.set_device(0)
    graphs = make_graphs("zinc", args.graphs)
    ds = DeviceDataset(graphs, device=torch.device("cuda", 0))
    loader = DataLoader(ds, batch_size=128, shuffle=True)
    torch.cuda.synchronize()
    n = sum(epoch_native(loader) for _ in range(args.trace_epochs))
    print(json.dumps({"trace": "native loader", "graphs": len(graphs), "fields": len(ds.field_names), "batch_size": 128, "epochs": args.trace_epochs,
                      "batches": n}), flush=True)


def summarise(args):
    """rocprofv3's --stats tables of a --trace-epochs run -> one csv: the kernels, then the memory copies."""
    rows = []
    for domain, pattern in (("KERNEL_DISPATCH", "*kernel_stats.csv"), ("MEMORY_COPY", "*memory_copy_stats.csv")):
        for path in sorted(glob.glob(os.path.join(args.summarise, "**", pattern), recursive=True)):
            with open(path, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.append([domain, r["Name"], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["Percentage"], r["MinNs"], r["MaxNs"]])
    if not rows:
        raise SystemExit("no *_stats.csv under %s" % args.summarise)
    os.makedirs(os.path.dirname(os.path.abspath(args.stats_out)), exist_ok=True)
    with open(args.stats_out, "w", newline="") as fh:
        w = csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Domain", "Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
        w.writerows(rows)
    for r in rows:
        print(",".join(str(c) for c in r[:4]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", nargs="+", default=["zinc", "molhiv"], choices=sorted(SHAPES))
    ap.add_argument("--batch-sizes", nargs="+", type=int, default=[32, 128, 1024, 4096])
    ap.add_argument("--graphs", type=int, default=None, help="graphs per dataset (default: 12 000 / 41 127)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-epochs", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--stats-out", default="profiles/loader_kernel_stats.csv")
    args = ap.parse_args()
    if args.summarise:
        summarise(args)
    elif args.trace_epochs:
        trace_epochs(args)
    else:
        bench(args)


if __name__ == "__main__":
    main()
