#!/usr/bin/env python3
"""Laplacian eigenvector fields on one GPU: graphs / s of ``dgn.laplacian_eigenvectors`` (csrc/eig.hip) on a molecule-shaped batch of
4 096 graphs (synth.zinc_shape_batch) for each Laplacian, device-event timing over windows of >= 1 s after a warm-up (the call with
device-resident inputs and check=False: what a training loop's preprocessing pays per batch), beside the reference's route on this
machine's CPU: scipy.sparse.linalg.eigs(L, k=4, which='SR', tol=1e-2) per graph (data/HIV.py:46), one thread, over 512 of those graphs.

    python scripts/bench_dgn_eig.py [--graphs 4096] [--window 1.0] [--scipy-graphs 512] [--out profiles/dgn_eig_bench.jsonl]

Prints one JSON line per measurement and appends it to ``--out``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gsn_amd import _abi, dgn, synth  # noqa: E402

NORMS = ("none", "sym", "walk")


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


def launch_alone(b, norm, window):
    """Seconds per launch of gsn_laplacian_eig_hip on pre-staged buffers (all graphs of `b` in one class, no host work but the call)."""
    n_class = next(c for c in dgn.EIG_CLASSES if c >= int(np.diff(b.node_ptr).max()))
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    npt, ept, ei = dv(b.node_ptr), dv(b.edge_ptr), dv(b.edge_index)
    G, N, E = b.num_graphs, b.num_nodes, b.num_edges
    vec, val = torch.empty(N, 4, device="cuda"), torch.empty(G, 4, device="cuda")
    status, sweeps = torch.zeros(G, dtype=torch.int32, device="cuda"), torch.zeros(G, dtype=torch.int32, device="cuda")
    n_scr = int(_abi.lib().gsn_laplacian_eig_scratch_floats(n_class, G))
    scratch = torch.empty(max(n_scr, 1), device="cuda")

    def call():
        _abi.check(_abi.lib().gsn_laplacian_eig_hip(G, _abi.ptr(npt), _abi.ptr(ept), _abi.ptr(ei), E, None, G, n_class, dgn.EIG_NORMS[norm], 4, 16,
                                                    _abi.ptr(vec), _abi.ptr(val), _abi.ptr(status), _abi.ptr(sweeps), _abi.ptr(scratch), n_scr,
                                                    _abi.current_stream()), "gsn_laplacian_eig_hip")
    s = timed(call, window)
    assert not bool(status.any())
    return s, n_class, int(sweeps.max())


def scipy_route(b, graphs, norm):
    """Seconds per graph of HIV.py:27-47 (sparse L, ARPACK) on the first `graphs` graphs with more than 5 vertices (HIV.py:65)."""
    from scipy import sparse as sp
    import scipy.sparse.linalg  # noqa: F401
    done, t = 0, 0.0
    for g in range(b.num_graphs):
        n, ei = b.graph(g)
        if n <= 5:
            continue
        t0 = time.perf_counter()
        A = sp.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n)).tocsr().astype(float)
        d = np.bincount(ei[1], minlength=n).clip(1)
        if norm == "none":
            L = sp.diags(d, dtype=float) * sp.eye(n) - A
        elif norm == "sym":
            N = sp.diags(d ** -0.5, dtype=float)
            L = sp.eye(n) - N * A * N
        else:
            L = sp.eye(n) - sp.diags(d ** -1.0, dtype=float) * A
        val, vec = sp.linalg.eigs(L, k=4, which="SR", tol=1e-2)
        np.real(vec[:, val.argsort()]).astype(np.float32)
        t += time.perf_counter() - t0
        done += 1
        if done == graphs:
            break
    return t / max(done, 1), done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--scipy-graphs", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dgn_eig_bench.jsonl"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    b = synth.zinc_shape_batch(args.graphs, seed=0)
    dev = synth.Batch(b.node_ptr, b.edge_ptr, b.edge_index)
    dev.edge_index = torch.from_numpy(b.edge_index).cuda()          # (node_ptr / edge_ptr stay on the host: the class grouping reads them)
    lines = []
    for norm in NORMS:
        vec, val, status, sweeps = dgn.laplacian_eigenvectors(dev, k=4, norm=norm, check=False, return_values=True, return_sweeps=True)
        assert not bool(status.any())
        s = timed(lambda: dgn.laplacian_eigenvectors(dev, k=4, norm=norm, check=False), args.window)
        lines.append(dict(what="laplacian_eigenvectors", native=True, norm=norm, k=4, graphs=b.num_graphs, nodes=b.num_nodes, edges=b.num_edges,
                          ms=s * 1e3, graphs_per_s=b.num_graphs / s, max_sweeps_used=int(sweeps.max())))
        print(json.dumps(lines[-1]), flush=True)
    # the launch alone, and the larger classes at batch scale (molecule-shaped trees with ring closures of 40 .. 64 / 80 .. 128 / 160 .. 256 vertices)
    shapes = [("molecules", b), ("n 40..64", synth.zinc_shape_batch(1024, seed=1, mean_n=52, sd_n=6, n_min=40, n_max=64, ring_rate=3.0)),
              ("n 80..128", synth.zinc_shape_batch(512, seed=2, mean_n=104, sd_n=12, n_min=80, n_max=128, ring_rate=6.0)),
              ("n 160..256", synth.zinc_shape_batch(64, seed=3, mean_n=208, sd_n=24, n_min=160, n_max=256, ring_rate=12.0))]
    for shape, bb in shapes:
        for norm in (NORMS if bb is b else ("none",)):
            s, n_class, most = launch_alone(bb, norm, args.window)
            lines.append(dict(what="gsn_laplacian_eig_hip_launch_alone", native=True, shape=shape, n_class=n_class, norm=norm, k=4,
                              graphs=bb.num_graphs, nodes=bb.num_nodes, ms=s * 1e3, graphs_per_s=bb.num_graphs / s, max_sweeps_used=most))
            print(json.dumps(lines[-1]), flush=True)
    for norm in NORMS:
        per, done = scipy_route(b, args.scipy_graphs, norm)
        lines.append(dict(what="scipy_eigs_tol1e-2_single_thread", native=False, norm=norm, k=4, graphs=done, us_per_graph=per * 1e6,
                          graphs_per_s=1.0 / per))
        print(json.dumps(lines[-1]), flush=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
