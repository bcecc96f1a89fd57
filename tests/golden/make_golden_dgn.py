#!/usr/bin/env python3
"""Generate tests/golden/dgn.<i>.npz: parity vectors of the directional GSN (directional_gsn/) from the REFERENCE's own Python.

Runs only where the reference tree is (like make_golden.py); the tests read the committed ``*.npz`` parts, never the reference.
The reference's nets/aggregators.py, scalers.py, layers.py, dgn_layer.py, mlp_readout_layer.py and
HIV_graph_classification/dgn_net.py are imported from where they lie; two things they import and this machine lacks are replaced
by stand-ins that live in this script:

* ``dgl`` -> a graph with ``ndata`` / ``edata``, ``apply_edges`` and ``update_all``, plus ``batch``, ``sum_nodes``, ``mean_nodes``,
  ``max_nodes``.  ``update_all`` reduces by in-degree buckets, the way DGL's degree bucketing does: the mailbox of a node holds its
  in-edges in edge-id order, and a node with no in-edge gets a zero row (DGL >= 0.5 zero-fills the reduced field of nodes that
  receive no message).  That last point is an ASSUMPTION (DGL is not installed here) -- INTEGRATION.md states it.
* ``ogb.graphproppred.mol_encoder`` -> AtomEncoder / BondEncoder: one xavier-initialised nn.Embedding per feature column, summed.

Usage:  python tests/golden/make_golden_dgn.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_golden import REF as REF_ROOT, save_parts  # noqa: E402

REF = os.path.join(REF_ROOT, "directional_gsn")
from gsn_amd import synth  # noqa: E402

ATOM_DIMS = [119, 4, 12, 12, 10, 6, 6, 2, 2]
BOND_DIMS = [5, 6, 2]


# ----------------------------------------------------------------------------------------------
# the dgl stand-in
# ----------------------------------------------------------------------------------------------
class _Edges:
    def __init__(self, g):
        self.src = {k: v[g.src] for k, v in g.ndata.items()}
        self.dst = {k: v[g.dst] for k, v in g.ndata.items()}
        self.data = dict(g.edata)


class _Nodes:
    def __init__(self, data, mailbox):
        self.data, self.mailbox = data, mailbox


class Graph:
    def __init__(self, src, dst, n, sizes=None):
        self.src, self.dst, self.n = torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64), int(n)
        self.ndata, self.edata = {}, {}
        self.sizes = [self.n] if sizes is None else list(sizes)

    def number_of_nodes(self):
        return self.n

    def apply_edges(self, fn):
        for k, v in fn(_Edges(self)).items():
            if v is not None:
                self.edata[k] = v

    def update_all(self, message_func, reduce_func):
        msgs = message_func(_Edges(self))
        deg = torch.bincount(self.dst, minlength=self.n)
        order = torch.argsort(self.dst, stable=True)          # in-edges of each node in edge-id order
        starts = torch.cumsum(deg, 0) - deg
        result = {}
        for D in sorted(set(deg.tolist()) - {0}):
            nodes = torch.nonzero(deg == D).flatten()
            idx = order[starts[nodes].unsqueeze(1) + torch.arange(D).unsqueeze(0)]        # [B, D] edge ids
            mailbox = {k: v[idx] for k, v in msgs.items()}
            out = reduce_func(_Nodes({k: v[nodes] for k, v in self.ndata.items()}, mailbox))
            for k, v in out.items():
                if k not in result:
                    result[k] = torch.zeros((self.n,) + tuple(v.shape[1:]), dtype=v.dtype)
                result[k] = result[k].index_copy(0, nodes, v)
        for k, v in result.items():
            self.ndata[k] = v


def _segments(g):
    return torch.repeat_interleave(torch.arange(len(g.sizes)), torch.tensor(g.sizes))


def sum_nodes(g, key):
    h = g.ndata[key]
    return torch.zeros(len(g.sizes), h.shape[1], dtype=h.dtype).index_add(0, _segments(g), h)


def mean_nodes(g, key):
    return sum_nodes(g, key) / torch.tensor(g.sizes, dtype=g.ndata[key].dtype).clamp(min=1).unsqueeze(1)


def max_nodes(g, key):
    h = g.ndata[key]
    idx = _segments(g).unsqueeze(1).expand(-1, h.shape[1])
    return torch.zeros(len(g.sizes), h.shape[1], dtype=h.dtype).scatter_reduce(0, idx, h, "amax", include_self=False)


class _FeatureEncoder(nn.Module):
    def __init__(self, emb_dim, dims, name):
        super().__init__()
        lst = nn.ModuleList()
        for dim in dims:
            e = nn.Embedding(dim, emb_dim)
            nn.init.xavier_uniform_(e.weight.data)
            lst.append(e)
        setattr(self, name, lst)
        self._name = name

    def forward(self, x):
        lst = getattr(self, self._name)
        return sum(lst[i](x[:, i]) for i in range(x.shape[1]))


def install_stubs():
    dgl = types.ModuleType("dgl")
    dgl.sum_nodes, dgl.mean_nodes, dgl.max_nodes = sum_nodes, mean_nodes, max_nodes
    dgl.nn = types.ModuleType("dgl.nn")
    dgl.nn.pytorch = types.ModuleType("dgl.nn.pytorch")
    dgl.nn.pytorch.glob = types.ModuleType("dgl.nn.pytorch.glob")
    dgl.nn.pytorch.glob.sum_nodes, dgl.nn.pytorch.glob.mean_nodes = sum_nodes, mean_nodes
    for name, m in [("dgl", dgl), ("dgl.nn", dgl.nn), ("dgl.nn.pytorch", dgl.nn.pytorch), ("dgl.nn.pytorch.glob", dgl.nn.pytorch.glob)]:
        sys.modules[name] = m
    me = types.ModuleType("ogb.graphproppred.mol_encoder")
    me.AtomEncoder = lambda emb_dim: _FeatureEncoder(emb_dim, ATOM_DIMS, "atom_embedding_list")
    me.BondEncoder = lambda emb_dim: _FeatureEncoder(emb_dim, BOND_DIMS, "bond_embedding_list")
    for name, m in [("ogb", types.ModuleType("ogb")), ("ogb.graphproppred", types.ModuleType("ogb.graphproppred")),
                    ("ogb.graphproppred.mol_encoder", me)]:
        sys.modules[name] = m


def import_reference():
    install_stubs()
    sys.path.insert(1, REF)
    import importlib
    mods = {n: importlib.import_module("nets." + n) for n in ["aggregators", "scalers", "layers", "dgn_layer", "mlp_readout_layer",
                                                              "HIV_graph_classification.dgn_net"]}
    for m in mods.values():
        assert m.__file__.startswith(REF), m.__file__
    return mods


# ----------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------
def odd_graph(rng):
    """A 40-node graph with an isolated node (39), in-degree-1 nodes, self loops, duplicate edges, and a tied neighbourhood:
    node 30's in-neighbours 31..34 carry identical dyadic rows (sums and squares exact in fp32)."""
    n = 40
    src = list(rng.integers(0, 30, size=90))
    dst = list(rng.integers(0, 30, size=90))
    src += [3, 3, 5, 7, 7, 11, 2, 31, 32, 33, 34, 35, 36]
    dst += [3, 8, 5, 9, 9, 11, 37, 30, 30, 30, 30, 38, 38]      # self loops 3, 5, 11; duplicate 7 -> 9; D = 1 at 37; 38 tied pair below
    return n, np.array([src, dst], dtype=np.int64)


def odd_features(rng, n, d):
    h = rng.standard_normal((n, d))
    h[31:35] = np.round(rng.standard_normal(d) * 8) / 8             # tied dyadic rows into node 30
    h[35] = h[36] = np.round(rng.standard_normal(d) * 4) / 4       # tied pair into node 38
    return h


def molecule_batch(num_graphs, seed):
    b = synth.zinc_shape_batch(num_graphs, seed=seed)
    rng = np.random.default_rng(seed + 1)
    codes = np.stack([rng.integers(0, min(dim, 5), size=b.num_nodes) for dim in ATOM_DIMS], 1).astype(np.int64)
    # an edge field shaped like GSN-e counts (id_scope local): symmetric small integers per undirected edge
    u, v = b.edge_index
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    ef = np.stack([(lo * 7 + hi * 13 + k * 5) % (3 + k) for k in range(3)], 1).astype(np.float32)
    return b, codes, ef


AGG_KINDS = ["mean", "sum", "max", "min", "std", "var", "dir1-av", "dir2-0.1", "dir2-neg-0.1", "dir1-dx", "dir0-dx", "dir1-dx-no-abs",
             "dir1-dx-balanced"]
SCALER_SETS = {"s1": "amplification", "s2": "identity amplification", "s3": "identity amplification attenuation"}


def run_aggregate(ref, g, h, nf, ef, aggregators, scalers, avg_log, dtype):
    """The reference's aggregation alone: pretrans_edges + update_all(message_func, reduce_func) of a DGNLayerSimple."""
    L = ref["dgn_layer"]
    layer = L.DGNLayer(in_dim=h.shape[1], out_dim=h.shape[1], dropout=0.0, graph_norm=False, batch_norm=False, aggregators=aggregators,
                       scalers=scalers, avg_d={"log": torch.tensor(avg_log, dtype=torch.float32)}, type_net="simple", residual=False).model
    g.ndata, g.edata = {}, {}
    ht = torch.tensor(h, dtype=dtype, requires_grad=True)
    g.ndata["h"] = ht
    if nf is not None:
        g.ndata["eig"] = torch.tensor(nf, dtype=dtype)
    if ef is not None:
        g.edata["eig"] = torch.tensor(ef, dtype=dtype)
    g.apply_edges(layer.pretrans_edges)
    g.update_all(layer.message_func, layer.reduce_func)
    out = g.ndata["h"]
    w = torch.tensor(np.random.default_rng(7).standard_normal(tuple(out.shape)), dtype=dtype)
    (out * w).sum().backward()
    return out.detach().numpy(), ht.grad.numpy(), w.numpy()


def gen_aggregate(ref, rec):
    rng = np.random.default_rng(0)
    n, ei = odd_graph(rng)
    d = 5
    h = odd_features(rng, n, d)
    nf = rng.integers(0, 4, size=(n, 3)).astype(np.float64)
    ef = rng.integers(-2, 3, size=(ei.shape[1], 2)).astype(np.float64)
    deg = np.bincount(ei[1], minlength=n)
    avg_log = float(np.mean(np.log(deg + 1.0)))
    g = Graph(ei[0], ei[1], n)
    rec["agg/edge_index"], rec["agg/h"], rec["agg/nf"], rec["agg/ef"] = ei, h, nf, ef
    rec["agg/avg_log"] = np.float32(avg_log)
    cases = []
    for fname, (f_n, f_e) in {"node": (nf, None), "edge": (None, ef), "both": (nf, ef)}.items():
        for sname, sc in SCALER_SETS.items():
            aggs = AGG_KINDS if fname != "edge" else [a for a in AGG_KINDS if not a.startswith("dir2")]   # (edge field: 2 columns)
            cases.append(("all_%s_%s" % (fname, sname), " ".join(aggs), sc, fname))
    for a in AGG_KINDS:
        cases.append(("one_%s" % a, a, SCALER_SETS["s3"], "both"))
    for name, aggs, sc, fname in cases:
        f_n = nf if fname in ("node", "both") else None
        f_e = ef if fname in ("edge", "both") else None
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            out, grad, w = run_aggregate(ref, g, h, f_n, f_e, aggs, sc, avg_log, dt)
            rec["agg/%s/out%s" % (name, tag)] = out
            rec["agg/%s/grad%s" % (name, tag)] = grad
        rec["agg/%s/w" % name] = w
        rec["agg/%s/aggregators" % name] = np.array(aggs)
        rec["agg/%s/scalers" % name] = np.array(sc)
        rec["agg/%s/fields" % name] = np.array(fname)
    rec["agg/cases"] = np.array([c[0] for c in cases])


LAYER_AGGS = "mean max min dir1-dx dir1-av"


def gen_layer(ref, rec):
    L = ref["dgn_layer"]
    b, _, ef = molecule_batch(6, seed=3)
    n, ei = b.num_nodes, b.edge_index
    d = 16
    rng = np.random.default_rng(5)
    h = rng.standard_normal((n, d)).astype(np.float32)
    sizes = np.diff(b.node_ptr)
    snorm = np.repeat(np.sqrt(1.0 / sizes.astype(np.float32)), sizes).astype(np.float32)[:, None]
    rec["layer/edge_index"], rec["layer/node_ptr"], rec["layer/h"], rec["layer/ef"], rec["layer/snorm_n"] = ei, b.node_ptr, h, ef, snorm
    cases = []
    for train in (True, False):
        for gn in (False, True):
            for res in (True, False):
                for pl in (1, 2):
                    cases.append("%s_gn%d_res%d_pl%d" % ("train" if train else "eval", gn, res, pl))
    for ci, case in enumerate(cases):
        train, gn, res, pl = case.startswith("train"), "gn1" in case, "res1" in case, int(case[-1])
        torch.manual_seed(100 + ci)
        layer = L.DGNLayer(in_dim=d, out_dim=d, dropout=0.0, graph_norm=gn, batch_norm=True, aggregators=LAYER_AGGS, scalers="identity",
                           avg_d={"log": torch.tensor(1.0)}, type_net="simple", residual=res, posttrans_layers=pl).model
        with torch.no_grad():
            layer.batchnorm_h.weight.uniform_(0.5, 1.5)
            layer.batchnorm_h.bias.uniform_(-0.5, 0.5)
            layer.batchnorm_h.running_mean.uniform_(-0.5, 0.5)
            layer.batchnorm_h.running_var.uniform_(0.5, 2.0)
        layer.train(train)
        sd = {k: v.detach().clone().numpy() for k, v in layer.state_dict().items()}
        g = Graph(ei[0], ei[1], n)
        g.edata["eig"] = torch.tensor(ef)
        ht = torch.tensor(h, requires_grad=True)
        y = layer(g, ht, None, torch.tensor(snorm))
        w = torch.tensor(np.random.default_rng(ci).standard_normal(tuple(y.shape)), dtype=torch.float32)
        (y * w).sum().backward()
        rec["layer/%s/y" % case] = y.detach().numpy()
        rec["layer/%s/w" % case] = w.numpy()
        rec["layer/%s/grad_h" % case] = ht.grad.numpy()
        for k, v in sd.items():
            rec["layer/%s/sd/%s" % (case, k)] = v
        for k, p in layer.named_parameters():
            rec["layer/%s/gp/%s" % (case, k)] = p.grad.numpy()
        if ci == 0:
            rec["names/layer_keys_pl1"] = np.array(list(sd))
        if case == "train_gn0_res1_pl2":
            rec["names/layer_keys_pl2"] = np.array(list(sd))
    rec["layer/cases"] = np.array(cases)


def gen_net(ref, rec):
    net_mod = ref["HIV_graph_classification.dgn_net"]
    b, codes, ef = molecule_batch(12, seed=11)
    n, ei = b.num_nodes, b.edge_index
    sizes = np.diff(b.node_ptr)
    deg = torch.tensor(np.bincount(ei[1], minlength=n), dtype=torch.float32)
    avg_d = dict(lin=torch.mean(deg), exp=torch.mean(torch.exp(torch.div(1, deg)) - 1), log=torch.mean(torch.log(deg + 1)))
    params = dict(L=4, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0,
                  dropout=0.0, graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av", scalers="identity",
                  towers=5, divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1, posttrans_layers=1,
                  pos_enc_dim=0, avg_d=avg_d, device="cpu")
    labels = np.random.default_rng(4).integers(0, 2, size=len(sizes)).astype(np.float32)
    snorm = np.repeat(np.sqrt(1.0 / sizes.astype(np.float32)), sizes).astype(np.float32)[:, None]
    rec["net/edge_index"], rec["net/node_ptr"], rec["net/codes"], rec["net/ef"], rec["net/labels"] = ei, b.node_ptr, codes, ef, labels
    rec["net/avg_log"] = np.float32(avg_d["log"])
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        torch.manual_seed(2024)
        net = net_mod.DGNNet(params).to(dt).train()
        if tag == "32":
            rec["names/net_keys"] = np.array(list(net.state_dict()))
            for k, v in net.state_dict().items():
                rec["net/sd/%s" % k] = v.detach().clone().numpy()
        else:
            net.load_state_dict({k: torch.tensor(rec["net/sd/%s" % k]).to(v.dtype) for k, v in net.state_dict().items()})
        opt = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=3e-6)
        g = Graph(ei[0], ei[1], n, sizes=sizes.tolist())
        g.edata["eig"] = torch.tensor(ef, dtype=dt)
        scores = net(g, torch.tensor(codes), None, torch.tensor(snorm, dtype=dt), None)
        loss = nn.BCEWithLogitsLoss()(scores, torch.tensor(labels, dtype=dt).unsqueeze(-1))
        opt.zero_grad()
        loss.backward()
        rec["net/scores%s" % tag] = scores.detach().numpy()
        rec["net/loss%s" % tag] = loss.detach().numpy()
        if tag == "64":
            # (the parameter-sized records: the fp64 run only, rounded to fp32 -- 6e-8 relative, far inside the tests' 2e-5 bar --
            #  which keeps the fixture near 2 MB)
            for k, p in net.named_parameters():
                rec["net/gp64/%s" % k] = p.grad.numpy().astype(np.float32)
            opt.step()
            for k, p in net.named_parameters():
                rec["net/step64/%s" % k] = p.detach().numpy().astype(np.float32)


def gen_net_variants(ref, rec):
    """The DGNNet paths the HIV config leaves out: a positional encoding (pos_enc_dim > 0: ndata['pos_enc'] through embedding_pos_enc)
    and the 'sum' / 'max' readouts; a small net (hidden 16, L = 2), fp64 forward scores and parameter gradients."""
    net_mod = ref["HIV_graph_classification.dgn_net"]
    b, codes, ef = molecule_batch(8, seed=21)
    n, ei = b.num_nodes, b.edge_index
    sizes = np.diff(b.node_ptr)
    pe = np.random.default_rng(22).standard_normal((n, 3)).astype(np.float32)
    snorm = np.repeat(np.sqrt(1.0 / sizes.astype(np.float32)), sizes).astype(np.float32)[:, None]
    labels = np.random.default_rng(23).integers(0, 2, size=len(sizes)).astype(np.float32)
    rec["netv/edge_index"], rec["netv/node_ptr"], rec["netv/codes"], rec["netv/ef"] = ei, b.node_ptr, codes, ef
    rec["netv/pos_enc"], rec["netv/labels"] = pe, labels
    readouts = ["sum", "max"]
    for ri, readout in enumerate(readouts):
        params = dict(L=2, hidden_dim=16, out_dim=16, type_net="simple", residual=True, edge_feat=False, readout=readout,
                      in_feat_dropout=0.0, dropout=0.0, graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av",
                      scalers="identity", towers=5, divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1,
                      posttrans_layers=1, pos_enc_dim=3, avg_d={"log": torch.tensor(1.0)}, device="cpu")
        torch.manual_seed(300 + ri)
        net = net_mod.DGNNet(params).train()
        for k, v in net.state_dict().items():
            rec["netv/%s/sd/%s" % (readout, k)] = v.detach().clone().numpy()
        net = net.double()
        g = Graph(ei[0], ei[1], n, sizes=sizes.tolist())
        g.edata["eig"] = torch.tensor(ef, dtype=torch.float64)
        g.ndata["pos_enc"] = torch.tensor(pe, dtype=torch.float64)
        scores = net(g, torch.tensor(codes), None, torch.tensor(snorm, dtype=torch.float64), None)
        loss = nn.BCEWithLogitsLoss()(scores, torch.tensor(labels, dtype=torch.float64).unsqueeze(-1))
        loss.backward()
        rec["netv/%s/scores64" % readout] = scores.detach().numpy()
        for k, p in net.named_parameters():
            rec["netv/%s/gp64/%s" % (readout, k)] = p.grad.numpy().astype(np.float32)
    rec["netv/readouts"] = np.array(readouts)


def main():
    torch.set_num_threads(4)
    ref = import_reference()
    rec = {}
    rec["names/aggregators"] = np.array(list(ref["aggregators"].AGGREGATORS))
    rec["names/scalers"] = np.array(list(ref["scalers"].SCALERS))
    gen_aggregate(ref, rec)
    gen_layer(ref, rec)
    gen_net(ref, rec)
    gen_net_variants(ref, rec)
    n = save_parts(HERE, "dgn", rec)
    print("dgn: %d arrays in %d parts" % (len(rec), n))


if __name__ == "__main__":
    main()
