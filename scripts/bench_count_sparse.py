"""Speed of the sparse counting kernel (gsn_count_sparse_hip, csrc/count_sparse.hip) on graphs the LDS-resident kernel refuses, and the
table of DESIGN.md section 3h.

Shapes: a hub graph (one vertex joined to 2 000 of 5 000, plus 5 000 random edges) and a sparse molecule-shaped graph of 5 000 vertices,
16 copies of each per launch; cycles 3-5, non-induced, vertex and edge mode.  Per shape and mode: ms per launch, graphs/s and the set-up /
search split.  The split is measured from outside: the set-up pass does not depend on the patterns, so a launch with the one-edge pattern
(whose cells end at once) times the set-up plus an empty search pass, and the rest of the full launch is search.  The only comparison there
is: the same family at 768 vertices on both kernels -- reported as a ratio, not gated on.

Digraph rows (a table of their own): random digraphs of 769 / 3 000, 1 000 / 5 000 and 900 / 9 000 vertices / arcs, a hub digraph of 1 200
vertices (500 out-spokes, 300 in-spokes, 2 500 random arcs), a molecule-shaped graph of 5 000 vertices with one random direction per edge,
and a 700-vertex digraph on both kernels; 16 graphs per launch, the digraph patterns of tests/golden/counts_directed.npz, non-induced,
vertex mode (there are no directed edge counts).

    python scripts/bench_count_sparse.py --out profiles/count_sparse_bench.jsonl     # on the GPU; also rewrites the table in DESIGN.md
    python scripts/bench_count_sparse.py --from-json profiles/count_sparse_bench.jsonl   # rewrite the table from recorded lines, no GPU
"""
import argparse
import json
import os
import sys
import time

import networkx as nx
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BEGIN, END = "<!-- bench_count_sparse:begin -->", "<!-- bench_count_sparse:end -->"
BEGIN_DIR, END_DIR = "<!-- bench_count_sparse_directed:begin -->", "<!-- bench_count_sparse_directed:end -->"
PATTERNS = [list(nx.cycle_graph(k).edges) for k in (3, 4, 5)]
ONE_EDGE = [[(0, 1)]]


def hub_graph(n, spokes, extra, seed):
    from gsn_amd import synth
    rng = np.random.default_rng(seed)
    und = {(0, int(v)) for v in rng.choice(np.arange(1, n), size=spokes, replace=False)}
    while len(und) < spokes + extra:
        a, b = (int(x) for x in rng.integers(1, n, size=2))
        if a != b:
            und.add((min(a, b), max(a, b)))
    return n, synth.undirected_to_edge_index(n, sorted(und))


def molecule_graph(n, seed):
    from gsn_amd import synth
    return synth.zinc_shape_graph(np.random.default_rng(seed), mean_n=n, sd_n=0.0, n_min=n, n_max=n, ring_rate=n / 16.0)


def digraph(n, arcs, seed, extra=None):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=arcs)
    ei = np.stack([src, (src + rng.integers(1, n, size=arcs)) % n]).astype(np.int64)
    return n, np.ascontiguousarray(ei if extra is None else np.concatenate([extra, ei], axis=1))


def hub_digraph(n, n_out, n_in, arcs, seed):
    rng = np.random.default_rng(seed)
    spokes = rng.choice(np.arange(1, n), size=n_out + n_in, replace=False)
    zero = np.zeros(n_out + n_in, np.int64)
    hub = np.concatenate([np.stack([zero[:n_out], spokes[:n_out]]), np.stack([spokes[n_out:], zero[n_out:]])], axis=1).astype(np.int64)
    return digraph(n, arcs, seed + 1000, extra=hub)


def oriented_molecule(n, seed):
    n, ei = molecule_graph(n, seed)
    ei = np.asarray(ei)
    ei = ei[:, ei[0] < ei[1]]
    flip = np.random.default_rng(seed).integers(0, 2, size=ei.shape[1]).astype(bool)
    return n, np.ascontiguousarray(np.where(flip[None, :], ei[::-1], ei).astype(np.int64))


def directed_patterns():
    z = np.load(os.path.join(REPO, "tests", "golden", "counts_directed.npz"))
    return [z["pattern/%d/edges" % i].tolist() for i in range(int(z["n_patterns"]))]


def timed(fn, window):
    import torch
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        t = time.perf_counter() - t0
        if t >= window and n >= 3:
            return t / n


def measure(window):
    import torch
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    lines = []
    shapes = [("hub: 1 vertex joined to 2 000 of 5 000, + 5 000 random edges", [hub_graph(5000, 2000, 5000, s) for s in range(16)]),
              ("molecule-shaped, 5 000 vertices", [molecule_graph(5000, s) for s in range(16)]),
              ("hub at 768 vertices (joined to 300, + 768 random edges)", [hub_graph(768, 300, 768, s) for s in range(16)]),
              ("molecule-shaped, 768 vertices", [molecule_graph(768, s) for s in range(16)])]
    for shape, graphs in shapes:
        b = synth.collate(graphs)
        ei = torch.from_numpy(b.edge_index).cuda()
        npt, ept = torch.from_numpy(b.node_ptr).cuda(), torch.from_numpy(b.edge_ptr).cuda()
        mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
        for mode in ("vertex", "edge"):
            plan, plan1 = CountPlan.get(PATTERNS, mode, False), CountPlan.get(ONE_EDGE, mode, False)
            rows = b.num_nodes if mode == "vertex" else b.num_edges
            out = torch.empty((rows, plan.n_cols), dtype=torch.int64, device="cuda")
            out1 = torch.empty((rows, plan1.n_cols), dtype=torch.int64, device="cuda")

            def run(p, o, large):
                # (max_nodes above 768 sends the launch straight to the sparse kernel; at 768 the sparse kernel is reached by saying so)
                return count_batch(p, npt, ept, ei, max_nodes=max(mn, 769) if large == "sparse" else mn, max_edges=me, out=o, check=False, large=large)

            full = timed(lambda: run(plan, out, "sparse"), window)
            setup = timed(lambda: run(plan1, out1, "sparse"), window)
            ln = dict(what="gsn_count_sparse_hip", shape=shape, mode=mode, graphs=b.num_graphs, nodes=b.num_nodes, columns=b.num_edges,
                      ms=full * 1e3, graphs_per_s=b.num_graphs / full, setup_ms=setup * 1e3, search_ms=max(full - setup, 0.0) * 1e3)
            if mn <= 768:
                ref = out.clone()
                lds = timed(lambda: run(plan, out, "refuse"), window)
                assert torch.equal(out, ref), "the two kernels disagree"
                ln.update(lds_ms=lds * 1e3, sparse_over_lds=full / lds)
            lines.append(ln)
            print(json.dumps(ln), flush=True)
    return lines


def measure_directed(window):
    import torch
    from gsn_amd import synth
    from gsn_amd.counting import CountPlan, count_batch
    lines = []
    shapes = [("random digraph, 769 vertices / 3 000 arcs", [digraph(769, 3000, s) for s in range(16)]),
              ("random digraph, 1 000 / 5 000", [digraph(1000, 5000, s) for s in range(16)]),
              ("random digraph, 900 / 9 000", [digraph(900, 9000, s) for s in range(16)]),
              ("hub digraph, 1 200 vertices: 500 out- and 300 in-spokes, + 2 500 random arcs", [hub_digraph(1200, 500, 300, 2500, s) for s in range(16)]),
              ("molecule-shaped, 5 000 vertices, one random direction per edge", [oriented_molecule(5000, s) for s in range(16)]),
              ("random digraph, 700 / 2 800", [digraph(700, 2800, s) for s in range(16)])]
    plan = CountPlan.get(directed_patterns(), "vertex", False, False, directed=True)
    plan1 = CountPlan.get(ONE_EDGE, "vertex", False, False, directed=True)
    for shape, graphs in shapes:
        b = synth.collate(graphs)
        ei = torch.from_numpy(b.edge_index).cuda()
        npt, ept = torch.from_numpy(b.node_ptr).cuda(), torch.from_numpy(b.edge_ptr).cuda()
        mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
        out = torch.empty((b.num_nodes, plan.n_cols), dtype=torch.int64, device="cuda")
        out1 = torch.empty((b.num_nodes, plan1.n_cols), dtype=torch.int64, device="cuda")

        def run(p, o, large):
            return count_batch(p, npt, ept, ei, max_nodes=max(mn, 769) if large == "sparse" else mn, max_edges=me, out=o, check=False, large=large)

        full = timed(lambda: run(plan, out, "sparse"), window)
        setup = timed(lambda: run(plan1, out1, "sparse"), window)
        ln = dict(what="gsn_count_sparse_hip", directed=True, shape=shape, mode="vertex", graphs=b.num_graphs, nodes=b.num_nodes, columns=b.num_edges,
                  ms=full * 1e3, graphs_per_s=b.num_graphs / full, setup_ms=setup * 1e3, search_ms=max(full - setup, 0.0) * 1e3)
        if mn <= 768:
            ref = out.clone()
            lds = timed(lambda: run(plan, out, "refuse"), window)
            assert torch.equal(out, ref), "the two kernels disagree"
            ln.update(lds_ms=lds * 1e3, sparse_over_lds=full / lds)
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    return lines


def table(lines):
    rows = ["| shape (16 graphs per launch) | mode | ms per launch | graphs/s | set-up ms | search ms | LDS kernel ms | sparse / LDS |", "|---|---|---|---|---|---|---|---|"]
    for ln in lines:
        lds = "%.2f" % ln["lds_ms"] if "lds_ms" in ln else "refused"
        ratio = "%.1f" % ln["sparse_over_lds"] if "lds_ms" in ln else "--"
        rows.append("| %s | %s | %.2f | %.0f | %.2f | %.2f | %s | %s |" % (ln["shape"], ln["mode"], ln["ms"], ln["graphs_per_s"], ln["setup_ms"], ln["search_ms"], lds, ratio))
    return "\n".join(rows)


def write_design(path, lines):
    text = open(path).read()
    for begin, end, part in ((BEGIN, END, [ln for ln in lines if not ln.get("directed")]), (BEGIN_DIR, END_DIR, [ln for ln in lines if ln.get("directed")])):
        if part and begin in text:
            a, b = text.index(begin) + len(begin), text.index(end)
            text = text[:a] + "\n" + table(part) + "\n" + text[b:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "count_sparse_bench.jsonl"))
    ap.add_argument("--from-json", default=None)
    ap.add_argument("--design", default=os.path.join(REPO, "DESIGN.md"))
    args = ap.parse_args()
    if args.from_json:
        lines = [json.loads(ln) for ln in open(args.from_json) if ln.strip()]
    else:
        lines = measure(args.window) + measure_directed(args.window)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    write_design(args.design, lines)


if __name__ == "__main__":
    main()
