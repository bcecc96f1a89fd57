#!/usr/bin/env python3
"""An evaluation epoch of the molhiv-shaped GNN_OGB two ways on the same box:

  reference   train_test_funcs.py:209-259 restated: per batch two .cpu() copies of predictions and labels, the boolean-index loss and its
              .item(); the metric from the gathered numpy arrays
  native      gsn_amd.evaluation.test_ogb: one gsn_eval_accumulate_hip call per batch, one host read at the end, the metric on the device

    python scripts/bench_evaluation.py [--batches 300] [--out profiles/evaluation_bench.jsonl]
    python scripts/bench_evaluation.py --loss-launches native|reference [--steps 100]     # under rocprofv3 --kernel-trace --stats: launches per loss

Both loops run the same model on the same batches (one synthetic batch per size, repeated: the forward's cost does not depend on the
contents) with a share of NaN labels; the metric of both is gsn_amd.evaluation.Evaluator (ogb is not a dependency), timed apart.
Prints one JSON line per batch size."""
import argparse
import importlib.util
import json
import os
import sys
import time
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from gsn_amd import evaluation as ev  # noqa: E402


def _train_script():
    spec = importlib.util.spec_from_file_location("train_step_molhiv", os.path.join(HERE, "train_step_molhiv.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Batch(types.SimpleNamespace):
    def to(self, device):
        return self


class Loader(list):
    def __init__(self, batch, n):
        super().__init__([batch] * n)
        self.dataset = range(n * batch.num_graphs)
        self.batch_size = batch.num_graphs


def reference_epoch(loader, model, loss_fn, device, evaluator):
    """the reference's test_ogb, line by line"""
    model.eval()
    y_true, y_pred, losses = [], [], []
    with torch.no_grad():
        for batch in loader:
            batch = batch.to(device)
            pred = model(batch)
            y_true.append(batch.y.view(pred.shape).cpu())
            y_pred.append(pred.cpu())
            y = batch.y.view(pred.shape)
            is_labeled = (y == y)
            loss = loss_fn(pred[is_labeled], y[is_labeled])
            losses.append(loss.item() * batch.num_graphs)
    t0 = time.perf_counter()
    metric = evaluator.eval({"y_true": torch.cat(y_true, dim=0).numpy(), "y_pred": torch.cat(y_pred, dim=0).numpy()})[evaluator.eval_metric]
    return sum(losses) / len(loader.dataset), metric, time.perf_counter() - t0


def epoch_bench(args, dev):
    ts = _train_script()
    lines = []
    for batch_size in (32, 128):
        a = types.SimpleNamespace(batch=batch_size, steps=1, warmup=1, layers=5, d=300, loss="masked", nan_share=0.2)
        model, data, _params, _opt, _loss, N, E = ts.build(a, dev)
        model.eval()
        batch = Batch(**vars(data), num_graphs=batch_size)
        loader = Loader(batch, args.batches)
        evaluator = ev.Evaluator("ogbg-molhiv")
        bce = torch.nn.BCEWithLogitsLoss()
        res = {}
        for name, fn in (("reference", lambda: reference_epoch(loader, model, bce, dev, evaluator)[:2]),
                         ("native", lambda: ev.test_ogb(loader, model, bce, dev, evaluator))):
            fn()                                                   # warm-up epoch (caches, allocator)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            times.sort()
            res[name] = dict(ms_per_epoch=round(times[len(times) // 2] * 1e3, 3), ms_min=round(times[0] * 1e3, 3), ms_max=round(times[-1] * 1e3, 3),
                             loss=out[0], rocauc=out[1])
        _, _, t_metric = reference_epoch(loader, model, bce, dev, evaluator)
        line = {"workload": "evaluation epoch, molhiv-shaped GNN_OGB (5 layers, d=300, vn), %d batches of %d graphs (N=%d, E=%d per batch), 20%% NaN labels"
                            % (args.batches, batch_size, N, E),
                "device": torch.cuda.get_device_name(dev), "arch": torch.cuda.get_device_properties(dev).gcnArchName,
                "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "repeats": args.repeats,
                "reference": res["reference"], "native": res["native"],
                "us_per_batch_reference": round(res["reference"]["ms_per_epoch"] * 1e3 / args.batches, 2),
                "us_per_batch_native": round(res["native"]["ms_per_epoch"] * 1e3 / args.batches, 2),
                "metric_ms_from_numpy_arrays": round(t_metric * 1e3, 3),
                "loss_difference": abs(res["reference"]["loss"] - res["native"]["loss"]),
                "rocauc_difference": abs(res["reference"]["rocauc"] - res["native"]["rocauc"])}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def loss_launches(args, dev):
    """`--steps` times the training-step loss and its backward on a [128, 1] batch with NaN labels: nothing but the loss launches kernels"""
    g = torch.Generator().manual_seed(0)
    y_hat = torch.randn(128, 1, generator=g).to(dev).requires_grad_(True)
    y = torch.randint(0, 2, (128, 1), generator=g).float()
    y[torch.rand(128, 1, generator=g) < 0.2] = float("nan")
    y = y.to(dev)
    bce = torch.nn.BCEWithLogitsLoss()
    for _ in range(args.steps):
        if args.loss_launches == "native":
            loss = ev.masked_loss("BCEWithLogitsLoss", y_hat, y)
        else:
            is_labeled = (y == y)
            loss = bce(y_hat[is_labeled], y[is_labeled])
        y_hat.grad = None
        loss.backward()
    torch.cuda.synchronize()
    print(json.dumps({"loss": args.loss_launches, "steps": args.steps, "value": float(loss)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--loss-launches", default="", choices=["", "native", "reference"])
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.loss_launches:
        loss_launches(args, dev)
    else:
        epoch_bench(args, dev)


if __name__ == "__main__":
    main()
