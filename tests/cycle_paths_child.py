"""Child process of tests/test_cycle_paths_gpu.py (not a test module): runs a fixed set of counting launches and saves every output --
int64 identifiers, fp32 encoded rows, fp16 pack columns (as bit patterns), status words -- into one .npz.  The parent runs it twice,
with GSN_COUNT_CYCLE=1 and =0 (the library reads the switch once per process), and compares the two files bit for bit.

usage: python cycle_paths_child.py OUT.npz"""
import os
import sys

import networkx as nx
import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gsn_amd import layers, packs, synth                                  # noqa: E402
from gsn_amd.counting import CountPlan, count_batch                        # noqa: E402
from gsn_amd.step import CountLayerStep                                    # noqa: E402

DEV = torch.device("cuda", 0)
CYCLES = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
CTOR = dict(d_in=28, d_ef=4, d_id=12, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128,
            d_up=128, d_h=[128], seed=0, activation_name="relu", bn=True, msg_kind="general")
OUT = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits16(x):
    return x.view(torch.int16).cpu().numpy()


def run_count(tag, plan, node_ptr, edge_ptr, ei, classes=(3, 3, 3, 3), clamp=True, max_nodes=None, max_edges=None):
    """count_batch three ways: counts + fp32 rows, counts + fp32 rows + pack columns, counts + pack columns only."""
    npt, ept, e = t(node_ptr), t(edge_ptr), t(ei)
    mn = int(np.diff(node_ptr).max()) if max_nodes is None else max_nodes
    me = int(np.diff(edge_ptr).max()) if max_edges is None else max_edges
    kw = dict(ids_are_global=True, max_nodes=mn, max_edges=me, device=DEV, check=False)
    ids, st, enc = count_batch(plan, npt, ept, e, encode=(list(classes), clamp), **kw)
    OUT[tag + "/ids"], OUT[tag + "/status"], OUT[tag + "/enc32"] = ids.cpu().numpy(), st.cpu().numpy(), enc.cpu().numpy()
    E = e.shape[1]
    pk = packs.new_edge_pack(E, DEV)
    ids, st, enc = count_batch(plan, npt, ept, e, encode=(list(classes), clamp), encoded_pack=(pk, 0), **kw)
    OUT[tag + "/p/ids"], OUT[tag + "/p/status"], OUT[tag + "/p/enc32"] = ids.cpu().numpy(), st.cpu().numpy(), enc.cpu().numpy()
    OUT[tag + "/p/pack"] = bits16(pk)
    pk = packs.new_edge_pack(E, DEV)
    ids, st, _ = count_batch(plan, npt, ept, e, encode=(list(classes), clamp), encoded_pack=(pk, 0), encoded_rows=False, **kw)
    OUT[tag + "/po/ids"], OUT[tag + "/po/status"], OUT[tag + "/po/pack"] = ids.cpu().numpy(), st.cpu().numpy(), bits16(pk)


def collate_raw(graphs):
    """[(n, edge_index [2, E] local ids)] -> node_ptr, edge_ptr, global edge_index; nothing is cleaned or checked."""
    node_ptr, edge_ptr, cols = [0], [0], []
    for n, ei in graphs:
        cols.append(np.asarray(ei, dtype=np.int64).reshape(2, -1) + node_ptr[-1])
        node_ptr.append(node_ptr[-1] + n); edge_ptr.append(edge_ptr[-1] + cols[-1].shape[1])
    return np.asarray(node_ptr, np.int64), np.asarray(edge_ptr, np.int64), np.ascontiguousarray(np.concatenate(cols, 1))


def both(und):
    und = np.asarray(und, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([und.T, und.T[::-1]], axis=1)


def main(path):
    plan = CountPlan.get(CYCLES, "edge", False)

    # (1) a ZINC-shaped batch of a few thousand graphs, an odd number of them
    b = synth.zinc_shape_batch(3001, seed=7)
    run_count("zinc", plan, b.node_ptr, b.edge_ptr, b.edge_index)
    run_count("zinc_unclamped", plan, b.node_ptr, b.edge_ptr, b.edge_index, classes=(2, 3, 2, 4), clamp=False)
    plan_perm = CountPlan.get([CYCLES[i] for i in (2, 0, 3, 1)], "edge", False)           # columns 5, 3, 6, 4
    run_count("zinc_perm", plan_perm, b.node_ptr, b.edge_ptr, b.edge_index, classes=(3, 2, 4, 3))

    # ... and through the one-call step (side workgroups: CSR, node pack, edge codes)
    torch.manual_seed(0)
    layer = layers.GSN_edge_sparse(flow="source_to_target", **CTOR).to(DEV).eval()
    step = CountLayerStep(plan, layer, [3, 3, 3, 3], clamp=True)
    mn, me = int(np.diff(b.node_ptr).max()), int(np.diff(b.edge_ptr).max())
    ids, y, st = step(t(b.node_ptr), t(b.edge_ptr), t(b.edge_index), layers.Codes(t(b.atom_type), [28]), layers.Codes(t(b.bond_type), [4]), mn, me)
    torch.cuda.synchronize()
    bufs = step._bufs[1]
    OUT["step/ids"], OUT["step/y"], OUT["step/status"] = ids.cpu().numpy(), y.cpu().numpy(), st.cpu().numpy()
    OUT["step/epack"], OUT["step/npack"] = bits16(bufs["epack"]), bits16(bufs["npack"])
    OUT["step/seg_ptr"], OUT["step/perm"] = bufs["seg_ptr"].cpu().numpy(), bufs["perm"].cpu().numpy()

    # (2) pairs that do not fit 64 vertices together: the one-by-one passes (and pairs that do fit, mixed in)
    rng = np.random.default_rng(3)
    sizes = [40, 45, 30, 20, 50, 20, 33, 33, 50, 48, 12, 14] * 180
    graphs = [synth.zinc_shape_graph(rng, mean_n=s, sd_n=0.0, n_min=s, n_max=s, ring_rate=s / 8.0) for s in sizes]
    node_ptr, edge_ptr, ei = collate_raw(graphs)
    assert np.diff(edge_ptr).max() <= 128
    run_count("wide_pairs", plan, node_ptr, edge_ptr, ei)

    # (3) self loops, duplicated columns, a missing reverse column (KeyError status), an out-of-range index (bad-index status), an empty
    # graph, dense little graphs -- 2101 graphs, odd, so that the last workgroup holds one graph
    ring6 = both([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3)])
    loops = np.concatenate([ring6, np.array([[1, 4, 0, 3], [1, 4, 1, 0]])], axis=1)        # two self loops, (0,1) and (3,0) again
    no_rev = ring6[:, ~((ring6[0] == 0) & (ring6[1] == 3))]                                # 3 -> 0 without 0 -> 3: on cycles
    pendant = np.concatenate([both([(0, 1), (1, 2), (2, 0)]), np.array([[2], [3]])], axis=1)  # one-way pendant: on no cycle, no error
    bad = ring6.copy(); bad[1, 4] = 9                                                      # vertex 9 of a 6-vertex graph
    k5, k7 = both(list(nx.complete_graph(5).edges)), both(list(nx.complete_graph(7).edges))
    specials = [(6, loops), (6, no_rev), (4, pendant), (6, bad), (5, np.zeros((2, 0), np.int64)), (5, k5), (7, k7), (6, ring6)]
    graphs = []
    for i in range(2101):
        if i % 9 == 4:
            graphs.append(specials[(i // 9) % len(specials)])
        else:
            n = int(rng.integers(3, 24))
            m = int(rng.integers(0, 30))
            u, v = rng.integers(0, n, m), rng.integers(0, n, m)                            # self loops and repeats included
            e = np.concatenate([np.stack([u, v]), np.stack([v, u])], 1)
            graphs.append((n, e[:, rng.permutation(e.shape[1])]))
    node_ptr, edge_ptr, ei = collate_raw(graphs)
    run_count("odd_lot", plan, node_ptr, edge_ptr, ei, classes=(3, 4, 4, 5))          # (16 classes: a whole edge-pack row)
    run_count("odd_lot_unclamped", plan, node_ptr, edge_ptr, ei, classes=(1, 2, 2, 3), clamp=False)
    np.savez(path, **OUT)


if __name__ == "__main__":
    main(sys.argv[1])
