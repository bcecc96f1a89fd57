#!/usr/bin/env python3
"""Native dropout (gsn_amd.dropout: one HIP launch per direction, the residual add included) beside the torch path it replaces, on one GPU
and in ONE call:

* forward + backward of ``F.dropout(x, p) + r`` against ``dropout(x, p, residual=r)`` on [837, 300] and [32, 300] (the node and graph rows of
  the molhiv B = 32 step) and [105 000, 300] (the config-4 step at 4 096 graphs), the two variants alternating round by round with device
  events around a block of repetitions; median and spread over the rounds.  Launches per call: the native ones through the
  ``flags.KERNEL_TIMER`` hook, the torch path's device kernels through the torch profiler;
* the molhiv B = 32 training step replayed as a HIP graph and the eager config-4 step at 4 096 graphs (scripts/train_step_molhiv.py) with
  ``--dropout torch`` against ``native``, alternating, ``--train-repeats`` runs each.

    python scripts/bench_dropout.py                      # everything; one JSON line per measurement, appended to profiles/dropout_bench.jsonl
    python scripts/bench_dropout.py --no-train           # the per-call table alone"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from gsn_amd import dropout as gdrop, flags  # noqa: E402

SHAPES = ((837, 300), (32, 300), (105000, 300))
OUT = None


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def block_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def call_table(dev, p, rounds, window):
    state = gdrop.DropoutState(dev, 1)
    for shape in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(shape, device=dev, generator=gen, requires_grad=True)
        r = torch.randn(shape, device=dev, generator=gen, requires_grad=True)
        g = torch.randn(shape, device=dev, generator=gen)

        def torch_call():
            torch.autograd.grad(F.dropout(x, p, True) + r, [x, r], g)

        def native_call():
            torch.autograd.grad(gdrop.dropout(x, p, True, r, state), [x, r], g)

        def graphed(fn):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            return graph

        graphs = {"torch": graphed(torch_call), "native": graphed(native_call)}
        fns = {("torch", "eager"): torch_call, ("native", "eager"): native_call,
               ("torch", "graph"): graphs["torch"].replay, ("native", "graph"): graphs["native"].replay}
        # launches per call: ours through the KERNEL_TIMER hook, ATen's device kernels through the profiler
        flags.KERNEL_TIMER = {}
        native_call()
        torch.cuda.synchronize(dev)
        launches = {"native": sum(len(v) for k, v in flags.KERNEL_TIMER.items() if k.startswith("dropout_"))}
        flags.KERNEL_TIMER = None
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
                torch_call()
                torch.cuda.synchronize(dev)
            launches["torch"] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as e:          # (a build without the device tracer: the count is not measured, the times are)
            launches["torch"] = None
            print("torch profiler: %s" % str(e).splitlines()[0], file=sys.stderr)
        reps = {}
        for key, fn in fns.items():                      # warm-up, and the repetitions that fill window / rounds seconds
            block_us(fn, 20)
            reps[key] = max(50, int(window / rounds / (block_us(fn, 50) * 1e-6)))
        times = {key: [] for key in fns}
        for _ in range(rounds):                          # the variants alternate: a drift of the machine hits all of them
            for key, fn in fns.items():
                times[key].append(block_us(fn, reps[key]))
        n = shape[0] * shape[1]
        for (variant, mode), ts in times.items():
            emit(what="dropout_residual_fwd_bwd", shape=list(shape), p=p, variant=variant, mode=mode, us_median=round(statistics.median(ts), 2),
                 us_min=round(min(ts), 2), us_max=round(max(ts), 2), rounds=rounds, reps_per_round=reps[(variant, mode)],
                 launches_per_call=launches[variant], bytes_moved_native=5 * 4 * n)      # x, r read, out written; grad_out read, grad_x written
        del graphs, fns


def train_steps(dev, repeats):
    mod = _script("train_step_molhiv")
    for what, base in (("molhiv_b32_graph_step", dict(batch=32, steps=200, warmup=3, layers=5, d=300, graph=True)),
                       ("config4_b4096_eager_step", dict(batch=4096, steps=10, warmup=2, layers=5, d=300, graph=False))):
        ms = {"torch": [], "native": []}
        for _ in range(repeats):
            for impl in ms:
                res = mod.run(types.SimpleNamespace(dropout=impl, **base), dev)
                assert res["dropout"] == impl
                ms[impl].append(res["ms_per_step"])
                torch.cuda.empty_cache()
        for impl, ts in ms.items():
            emit(what=what, dropout=impl, batch=base["batch"], launch="hip_graph" if base["graph"] else "eager",
                 ms_median=round(statistics.median(ts), 4), ms_min=min(ts), ms_max=max(ts), runs=ts, steps=base["steps"])


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of repetitions per variant, over all rounds")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "dropout_bench.jsonl"), help="JSON lines are appended here ('' for none)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dropout.py measures on the GPU; there is no CPU fallback"
    OUT = a.out or None
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    call_table(dev, a.p, a.rounds, a.window)
    if not a.no_train:
        train_steps(dev, a.train_repeats)


if __name__ == "__main__":
    main()
