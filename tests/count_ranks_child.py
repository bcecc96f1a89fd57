"""Child process of tests/test_count_ranks_gpu.py (not a test module): count_batch over the cases of tests/count_ranks_cases.py, int64
identifiers and status words into one .npz.  The parent starts it with GSN_COUNT_CYCLE=0 (the library reads the switch once per process):
every launch here is the plan interpreter's, the reference the cycle instantiation is compared to bit for bit.

usage: python count_ranks_child.py OUT.npz"""
import os
import sys

import networkx as nx
import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from count_ranks_cases import ALL_CASES, count_case                         # noqa: E402
from gsn_amd.counting import CountPlan, count_batch                         # noqa: E402


def main(path):
    dev = torch.device("cuda", 0)
    plan = CountPlan.get([list(nx.cycle_graph(k).edges) for k in range(3, 7)], "edge", False)
    out = {}
    for name in ALL_CASES:
        node_ptr, edge_ptr, ei, glob, mn, me = count_case(name)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ids, st = count_batch(plan, t(node_ptr), t(edge_ptr), t(ei), ids_are_global=glob, max_nodes=mn, max_edges=me, device=dev, check=False)
        out[name + "/ids"], out[name + "/status"] = ids.cpu().numpy(), st.cpu().numpy()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
