#!/usr/bin/env python3
"""Generate tests/golden/dgn_eig.npz: what the REFERENCE's own ``positional_encoding`` (directional_gsn/data/HIV.py:21-51) computes on
a dozen small graphs, for its three Laplacians.

Runs only where the reference tree is (like make_golden_dgn.py); the tests read the committed ``dgn_eig.npz``, never the reference.
``data/HIV.py`` is imported from where it lies, over stand-ins for what this machine lacks:

* ``dgl`` -> ``dgl.backend.asnumpy`` and a graph with ``ndata``, ``number_of_nodes``, ``in_degrees`` and ``adjacency_matrix_scipy``
  (A[u, v] = number of arcs u -> v: a COO matrix of ones, whose conversion to CSR adds duplicates);
* ``ogb.graphproppred`` (dataset classes ``HIV.py`` only names) and the two ``utils_*`` modules it imports but ``positional_encoding``
  does not use.

``scipy.sparse.linalg.eigs`` is wrapped so that the ``L`` the reference hands to ARPACK is recorded densely, together with the
eigenvalues ARPACK returned.  Stored per case ``<graph>/<norm>``: the edge list, ``L``, the returned [n, 4] tensor, the returned
eigenvalues (sorted), and per reference vector r its own deviation ``delta = |r - P_C r|_2`` from the exact (float64 ``eigh``) eigenspace
of the cluster its eigenvalue belongs to -- the reference calls ARPACK with ``tol=1e-2``, so that error is measured here, not assumed.

Usage:  python tests/golden/make_golden_dgn_eig.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import scipy.sparse
import scipy.sparse.linalg
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_golden import REF as REF_ROOT  # noqa: E402
import make_golden_dgn as mg  # noqa: E402  (the dgl / ogb stand-ins of the DGN generator)
import dgn_eig_ref as R  # noqa: E402

HIV = os.path.join(REF_ROOT, "directional_gsn", "data", "HIV.py")


class Graph(mg.Graph):
    def in_degrees(self):
        return torch.bincount(self.dst, minlength=self.n)

    def adjacency_matrix_scipy(self, return_edge_ids=False):
        ones = np.ones(len(self.src), dtype=np.int64)
        return scipy.sparse.coo_matrix((ones, (self.src.numpy(), self.dst.numpy())), shape=(self.n, self.n)).tocsr()


def import_reference():
    mg.install_stubs()
    dgl = sys.modules["dgl"]
    dgl.backend = types.ModuleType("dgl.backend")
    dgl.backend.asnumpy = lambda t: t.numpy()
    sys.modules["dgl.backend"] = dgl.backend
    gp = sys.modules["ogb.graphproppred"]
    gp.DglGraphPropPredDataset = gp.Evaluator = object
    for name, attr in (("utils_subgraph_encoding", "prepare_dataset"), ("utils_one_hot_encoding", "encode")):
        m = types.ModuleType(name)
        setattr(m, attr, None)
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("reference_HIV", HIV)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    g = dict(R.known_graphs())
    g["tree10"] = R.tree_with_rings(10, 0)
    g["tree17"] = R.tree_with_rings(17, 0)
    g["tree24"] = R.tree_with_rings(24, 0)
    return g


def main():
    ref = import_reference()
    recorded = {}
    real_eigs = scipy.sparse.linalg.eigs

    def eigs(L, *a, **kw):
        val, vec = real_eigs(L, *a, **kw)
        recorded["L"] = np.asarray(L.toarray(), dtype=np.float64)
        recorded["val"] = np.sort(np.real(val))
        return val, vec

    scipy.sparse.linalg.eigs = eigs
    ref.sp.linalg.eigs = eigs
    out = {}
    names = []
    for name, (n, ei) in cases().items():
        for norm in R.NORMS:
            g = Graph(ei[0], ei[1], n)
            g = ref.positional_encoding(g, 4, norm)
            vec = g.ndata["eig"].numpy()
            assert vec.shape == (n, 4) and vec.dtype == np.float32
            L = recorded["L"]
            lam, U = R.truth(n, ei, norm)
            F = float(np.linalg.norm(L))
            delta = np.zeros(4)
            for j in range(4):
                pos = int(np.argmin(np.abs(lam - recorded["val"][j])))
                lo, hi, _ = R.cluster_of(lam, F, pos)
                delta[j] = R.off_space(vec[:, j].astype(np.float64), U[:, lo:hi])
            key = "%s/%s" % (name, norm)
            names.append(key)
            out[key + "/edge_index"] = ei.astype(np.int64)
            out[key + "/n"] = np.int64(n)
            out[key + "/L"] = L
            out[key + "/eig"] = vec
            out[key + "/val"] = recorded["val"]
            out[key + "/delta"] = delta
            print("%-28s n=%2d  val %s  delta %s" % (key, n, np.round(recorded["val"], 4), np.array2string(delta, precision=2)))
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "dgn_eig.npz"), **out)
    print("wrote dgn_eig.npz: %d cases, %d bytes" % (len(names), os.path.getsize(os.path.join(HERE, "dgn_eig.npz"))))


if __name__ == "__main__":
    main()
