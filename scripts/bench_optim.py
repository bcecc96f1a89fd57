#!/usr/bin/env python3
"""Time per optimizer step: gsn_amd.optim.Adam (one HIP launch) beside torch.optim.Adam(capturable=True) and, where this build constructs
it, torch.optim.Adam(fused=True, capturable=True) -- on the parameter lists of the config-2 model (GNNSubstructures 4 x 128,
scripts/train_step_zinc.py) and the config-4 model (GNN_OGB 5 x 300 + virtual node, scripts/train_step_molhiv.py), with random gradients,
each variant eager and as a captured step-only HIP graph.  All variants are measured in ONE call, alternating round by round, with device
events around a block of repetitions; the spread over the rounds is reported beside the median.

    python scripts/bench_optim.py                      # the step-only table, then the --graph training steps with adam / adam_native
    python scripts/bench_optim.py --no-train           # the step-only table alone
    python scripts/bench_optim.py --loop native:molhiv:500      # nothing but 500 eager steps of one variant: run it under
                                                                # `rocprofv3 --kernel-trace --stats` to count the launches per step
    python scripts/bench_optim.py --summarise stats.csv --steps 500      # launches per step out of that run's kernel statistics

One JSON line per measurement."""
import argparse
import csv
import importlib.util
import json
import os
import statistics
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from gsn_amd import optim  # noqa: E402

VARIANTS = ("torch_capturable", "torch_fused", "native")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(model, **kw):
    base = dict(batch=128, steps=1, warmup=1) if model == "zinc" else dict(batch=32, steps=1, warmup=1, layers=5, d=300)
    return types.SimpleNamespace(**dict(base, **kw))


def parameter_shapes(model, dev):
    """The parameter list of the training script's build(), as shapes (the model itself is dropped again)."""
    mod = _script("train_step_zinc" if model == "zinc" else "train_step_molhiv")
    params = mod.build(_args(model), dev)[2]
    return [tuple(p.shape) for p in params]


def make_variant(variant, shapes, dev, seed=0):
    """(optimizer, parameters) with fixed random gradients, or None when this build does not construct the variant."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.1) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
    try:
        if variant == "native":
            opt = optim.Adam(params, lr=1e-3)
        elif variant == "torch_fused":
            opt = torch.optim.Adam(params, lr=1e-3, fused=True, capturable=True)
        else:
            opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        opt.step()
    except (RuntimeError, ValueError, TypeError) as e:
        if variant == "native":
            raise
        print(json.dumps({"what": "optimizer_step", "variant": variant, "skipped": str(e).splitlines()[0]}), flush=True)
        return None
    return opt, params


def captured(opt, dev):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    return graph


def block_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def step_table(dev, rounds, window):
    for model in ("zinc", "molhiv"):
        shapes = parameter_shapes(model, dev)
        n_elems = sum(int(torch.Size(s).numel()) for s in shapes)
        fns, keep = {}, []
        for variant in VARIANTS:
            made = make_variant(variant, shapes, dev)
            if made is None:
                continue
            fns[(variant, "eager")] = made[0].step
            made_g = make_variant(variant, shapes, dev)
            graph = captured(made_g[0], dev)
            fns[(variant, "graph")] = graph.replay
            keep += [made, made_g, graph]
        reps = {}
        for key, fn in fns.items():                      # warm-up, and the repetitions that fill window / rounds seconds
            block_us(fn, 20)
            reps[key] = max(50, int(window / rounds / (block_us(fn, 50) * 1e-6)))
        times = {key: [] for key in fns}
        for _ in range(rounds):                          # the variants alternate: a drift of the machine hits all of them
            for key, fn in fns.items():
                times[key].append(block_us(fn, reps[key]))
        for (variant, mode), ts in times.items():
            print(json.dumps({"what": "optimizer_step", "model": model, "tensors": len(shapes), "elements": n_elems, "variant": variant, "mode": mode,
                              "us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                              "rounds": rounds, "reps_per_round": reps[(variant, mode)]}), flush=True)
        del fns, keep


def train_steps(dev, repeats, steps):
    """The --graph training steps of the two scripts with --optimizer adam against adam_native, alternating, `repeats` runs each."""
    for model, name in (("molhiv", "train_step_molhiv"), ("zinc", "train_step_zinc")):
        mod = _script(name)
        ms = {"adam": [], "adam_native": []}
        for _ in range(repeats):
            for o in ms:
                res = mod.run(_args(model, steps=steps, warmup=3, graph=True, optimizer=o), dev)
                ms[o].append(res["ms_per_step"])
        for o, ts in ms.items():
            print(json.dumps({"what": "train_step_graph", "model": model, "batch": _args(model).batch, "optimizer": o, "ms_median": round(statistics.median(ts), 4),
                              "ms_min": min(ts), "ms_max": max(ts), "runs": ts, "steps": steps}), flush=True)


def loop(spec, dev):
    variant, model, steps = spec.split(":")
    made = make_variant({"native": "native", "fused": "torch_fused", "capturable": "torch_capturable"}.get(variant, variant), parameter_shapes(model, dev), dev)
    if made is None:
        return
    for _ in range(int(steps) - 1):                     # (make_variant has taken the first step)
        made[0].step()
    torch.cuda.synchronize(dev)
    print(json.dumps({"what": "loop", "variant": variant, "model": model, "steps": int(steps)}), flush=True)


def summarise(path, steps):
    """Kernels of a `rocprofv3 --kernel-trace --stats` run that ran at least once per step, and their launches per step."""
    rows = list(csv.DictReader(open(path)))
    per_step, total = [], 0.0
    for r in rows:
        calls = int(r.get("Calls") or r.get("calls") or 0)
        if calls >= steps:
            per_step.append((r.get("Name") or r.get("name"), calls))
            total += calls / steps
    for name, calls in per_step:
        print("%8d calls  %6.2f per step  %s" % (calls, calls / steps, name[:150]))
    print("launches per step (kernels with >= %d calls): %.2f" % (steps, total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of repetitions per variant, over all rounds")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-repeats", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--loop", default=None, help="VARIANT:MODEL:STEPS -- eager steps of one variant and nothing else (for a kernel trace)")
    ap.add_argument("--summarise", default=None, help="kernel statistics CSV of a traced --loop run")
    ap.add_argument("--steps", type=int, default=500, help="with --summarise: the steps of the traced loop")
    a = ap.parse_args()
    if a.summarise is not None:
        return summarise(a.summarise, a.steps)
    assert torch.cuda.is_available(), "bench_optim.py measures on the GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if a.loop:
        return loop(a.loop, dev)
    step_table(dev, a.rounds, a.window)
    if not a.no_train:
        train_steps(dev, a.train_repeats, a.train_steps)


if __name__ == "__main__":
    main()
