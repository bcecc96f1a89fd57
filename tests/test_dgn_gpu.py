"""Directional GSN on the GPU (gsn_amd.dgn, csrc/dgn.hip): the aggregation kernels against the reference's own code (fixtures from
tests/golden/make_golden_dgn.py) and against an fp64 restatement on molecule-shaped batches; the layer and DGNNet against the fixtures;
determinism, graph capture, empty batches."""
import numpy as np
import pytest
import torch

from helpers import load

pytestmark = pytest.mark.gpu

EPS = 1e-8
TOL = 1e-5
GTOL = 2e-5
DEV = "cuda"


def elementwise_ok(got, ref, rtol=TOL):
    """|got - ref| <= rtol |ref| + rtol * max|ref row|, every element"""
    got, ref = got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return bool(((got - ref).abs() <= rtol * ref.abs() + rtol * ref.abs().amax(dim=1, keepdim=True)).all())


def _z():
    return load("dgn")


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ------------------------------------------------------------------------------------------------------------------
# fp64 restatement of dgn_layer.py:38-56 over an edge list (scatter_reduce / index_add)
# ------------------------------------------------------------------------------------------------------------------
def restate(h, ei, nf, ef, aggregators, scalers, avg_log):
    """The layer's aggregation output [N, S*A*d] in h's dtype (autograd flows through it)."""
    from gsn_amd import dgn
    N, d = h.shape
    src, dst = ei[0], ei[1]
    D = torch.bincount(dst, minlength=N).to(h.dtype)
    has = (D > 0).unsqueeze(1)
    Dc = D.clamp(min=1).unsqueeze(1)
    parts = []
    if nf is not None:
        parts.append(nf[src] - nf[dst])
    if ef is not None:
        parts.append(ef)
    vf = torch.cat(parts, 1) if parts else None
    hs = h[src]
    z = lambda: torch.zeros(N, d, dtype=h.dtype, device=h.device)
    seg = lambda x: torch.zeros(N, *x.shape[1:], dtype=h.dtype, device=h.device).index_add(0, dst, x)
    idx = dst.unsqueeze(1).expand(-1, d)
    out = []
    for name in aggregators.split():
        kind, col, alpha = dgn.AGGREGATORS[name]
        if kind == dgn.MEAN:
            y = seg(hs) / Dc
        elif kind == dgn.SUM:
            y = seg(hs)
        elif kind in (dgn.MAX, dgn.MIN):
            y = z().scatter_reduce(0, idx, hs, "amax" if kind == dgn.MAX else "amin", include_self=False)
        elif kind in (dgn.VAR, dgn.STD):
            m1 = seg(hs) / Dc
            var = torch.relu(seg(hs * hs) / Dc - m1 * m1)
            y = var if kind == dgn.VAR else torch.sqrt(var + EPS)
        else:
            w = vf[:, col]
            if kind == dgn.DIR_SOFTMAX:
                x = alpha * w.abs()
                m = torch.full((N,), -float("inf"), dtype=h.dtype, device=h.device).scatter_reduce(0, dst, x, "amax")
                ex = torch.exp(x - m[dst])
                wt = ex / seg(ex.unsqueeze(1))[dst, 0]
            elif kind == dgn.DIR_DX_BALANCED:
                pos, neg = torch.relu(w), torch.relu(-w)
                wt = (pos / (seg(pos.unsqueeze(1))[dst, 0] + EPS) + neg / (seg(neg.unsqueeze(1))[dst, 0] + EPS)) / 2
            else:
                wt = (w.abs() if kind == dgn.DIR_AV else w) / (seg(w.abs().unsqueeze(1))[dst, 0] + EPS)
            y = seg(hs * wt.unsqueeze(1))
            if kind in (dgn.DIR_DX, dgn.DIR_DX_NOABS, dgn.DIR_DX_BALANCED):
                y = y - seg(wt.unsqueeze(1)) * h
                if kind != dgn.DIR_DX_NOABS:
                    y = y.abs()
        out.append(torch.where(has, y, torch.zeros_like(y)))
    cat = torch.cat(out, 1)
    sc = scalers.split()
    if len(sc) > 1:
        lg = torch.log(D + 1).unsqueeze(1)
        f = {"identity": torch.ones_like(lg), "amplification": lg / avg_log, "attenuation": avg_log / lg}
        cat = torch.cat([cat * torch.where(has, f[s], torch.zeros_like(lg)) for s in sc], 1)
    return cat


def kinds_of(aggregators, scalers, d):
    names = aggregators.split()
    S = len(scalers.split()) if len(scalers.split()) > 1 else 1
    return [names[j] for s in range(S) for j in range(len(names)) for _ in range(d)]


def check_forward(got, ref64, aggregators, scalers, h64, ei, d):
    """elementwise_ok at 1e-5 with the row floor; std / var columns in the variance domain: |got^2 - EPS - var64| <= 1e-5 rowmax(mean h^2)."""
    kinds = np.array(kinds_of(aggregators, scalers, d))
    sv = torch.from_numpy(np.isin(kinds, ["std", "var"])).to(got.device)
    rest = ~sv
    ok = elementwise_ok(got[:, rest].double(), ref64[:, rest]) if rest.any() else True
    if sv.any():
        N = h64.shape[0]
        D = torch.bincount(ei[1], minlength=N).double().clamp(min=1).unsqueeze(1)
        m2 = torch.zeros_like(h64).index_add(0, ei[1], h64[ei[0]] ** 2) / D
        floor = TOL * m2.amax(1, keepdim=True) + 1e-30
        is_std = torch.from_numpy(kinds == "std").to(got.device)
        g = got.double()
        var_got = torch.where(is_std, g * g - EPS, g)
        var_ref = torch.where(is_std, ref64 * ref64 - EPS, ref64)
        ok = ok and bool(((var_got - var_ref)[:, sv].abs() <= floor).all())
    return ok


# ------------------------------------------------------------------------------------------------------------------
# (a) / (b) against the reference's own code
# ------------------------------------------------------------------------------------------------------------------
def _agg_case(z, case):
    from gsn_amd import dgn
    fields = str(z["agg/%s/fields" % case])
    nf = _t(z["agg/nf"]) if fields in ("node", "both") else None
    ef = _t(z["agg/ef"]) if fields in ("edge", "both") else None
    return (str(z["agg/%s/aggregators" % case]), str(z["agg/%s/scalers" % case]), nf, ef,
            {"log": float(z["agg/avg_log"])}, dgn)


@pytest.mark.parametrize("case", [str(c) for c in load("dgn")["agg/cases"]])
def test_aggregate_matches_reference(case):
    z = _z()
    aggs, sc, nf, ef, avg_d, dgn = _agg_case(z, case)
    ei = _t(z["agg/edge_index"], torch.int64)
    h = _t(z["agg/h"]).requires_grad_(True)
    y = dgn.dgn_aggregate(h, ei, aggs, sc, avg_d, node_field=nf, edge_field=ef)
    ref64 = _t(z["agg/%s/out64" % case], torch.float64)
    assert y.shape == ref64.shape
    assert check_forward(y.detach(), ref64, aggs, sc, _t(z["agg/h"], torch.float64), ei, h.shape[1]), case
    (y * _t(z["agg/%s/w" % case])).sum().backward()
    g64 = _t(z["agg/%s/grad64" % case], torch.float64)
    assert elementwise_ok(h.grad.double(), g64, GTOL), (case, float((h.grad.double() - g64).abs().max()))
    # the fixture's special nodes: isolated node 39 has a zero row; D = 1 (node 37) and the tied neighbourhoods (30, 38) give
    # std == sqrt(EPS) exactly
    yd = y.detach()
    assert float(yd[39].abs().max()) == 0.0
    names = aggs.split()
    if "std" in names and len(sc.split()) == 1:
        j = names.index("std")
        d = h.shape[1]
        s = float(np.sqrt(np.float32(EPS)))                     # (correctly rounded fp32 sqrt)
        for v in (30, 37, 38):
            assert torch.all(yd[v, j * d:(j + 1) * d] == s), (case, v)


# ------------------------------------------------------------------------------------------------------------------
# (a) / (b) against the fp64 restatement on molecule-shaped batches of >= 100 k nodes
# ------------------------------------------------------------------------------------------------------------------
_BIG = {}


def _molecules():
    if "b" not in _BIG:
        from gsn_amd import synth
        b = synth.zinc_shape_batch(4600, seed=7)              # > 100 k atoms
        ei = torch.from_numpy(b.edge_index).to(DEV)
        rng = np.random.default_rng(3)
        u, v = b.edge_index
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        ef = np.stack([(lo * 7 + hi * 13 + k) % (3 + k) for k in range(2)], 1).astype(np.float32) - 1.0   # signed, symmetric
        nf = rng.integers(0, 4, size=(b.num_nodes, 2)).astype(np.float32)
        _BIG["b"] = (b, ei, _t(nf), _t(ef))
    return _BIG["b"]


def _tie_free(N, d, seed):
    """Rows with no two equal values in any column (a permutation of a grid per column, jittered within its cell so that no exact
    linear relation between grid values puts a dx aggregator exactly on its abs kink): max / min have one arg each."""
    g = torch.Generator().manual_seed(seed)
    cols = [(torch.randperm(N, generator=g).double() + 0.1 + 0.8 * torch.rand(N, generator=g, dtype=torch.float64)) / N * 4 - 2
            for _ in range(d)]
    return torch.stack(cols, 1).float().double().to(DEV)


BIG_AGGS = "mean sum max min std var dir0-av dir1-0.1 dir2-neg-0.1 dir1-dx dir2-dx-no-abs dir3-dx-balanced"


@pytest.mark.parametrize("d,layout", [(1, "aligned"), (3, "aligned"), (70, "aligned"), (128, "aligned"), (300, "aligned"), (70, "offset")])
def test_aggregate_vs_fp64_molecules(d, layout):
    """d = 300 (float4 rows, 75 per row > 64 lanes) and d = 70 rows starting 4 bytes into their buffer (1 float per lane, 70 > 64)
    take two feature chunks per lane: the statistics are recomputed per chunk."""
    from gsn_amd import dgn
    b, ei, nf, ef = _molecules()
    N = b.num_nodes
    assert N >= 100000
    h64 = _tie_free(N, d, d)
    sc = "identity amplification attenuation" if d in (3, 70) else "identity"
    avg = {"log": float(dgn.avg_degree_log(b))}
    if layout == "offset":
        buf = torch.empty(N * d + 1, device=DEV)
        h = buf[1:].view(N, d)
        h.copy_(h64.float())
        assert h.is_contiguous() and h.data_ptr() % 8 == 4      # (rows only 4-byte aligned: the kernel takes 1 float per lane)
        h.requires_grad_(True)
    else:
        h = h64.float().requires_grad_(True)
    y = dgn.dgn_aggregate(h, ei, BIG_AGGS, sc, avg, node_field=nf, edge_field=ef)
    hr = h.detach().double().requires_grad_(True)
    ref = restate(hr, ei, nf.double(), ef.double(), BIG_AGGS, sc, torch.tensor(avg["log"], dtype=torch.float32).double())
    assert check_forward(y.detach(), ref.detach(), BIG_AGGS, sc, hr.detach(), ei, d)
    # gradients: std / var columns get no upstream gradient here.  Their adjoint 2 (h_k - m1) / (D std) is ill-conditioned where a
    # neighbourhood's variance is within fp32 cancellation of zero (std ~ sqrt(EPS)), which a batch this size always contains; the
    # fixtures above check them against the reference's own fp32 and fp64 runs
    # and the |T| of the dx kinds gets none where T is within fp32 rounding of the abs kink (|T| < 1e-5: a handful of elements), where
    # the two evaluations may legitimately take opposite signs
    kinds = np.array(kinds_of(BIG_AGGS, sc, d))
    keep = torch.from_numpy(~np.isin(kinds, ["std", "var"])).to(DEV).expand_as(y)
    kink = torch.from_numpy(np.isin(kinds, ["dir1-dx", "dir3-dx-balanced"])).to(DEV) & (ref.detach().abs() < 1e-5)
    w = torch.randn_like(y) * (keep & ~kink)
    (y * w).sum().backward()
    (ref * w.double()).sum().backward()
    err = float((h.grad.double() - hr.grad).abs().max()) / float(hr.grad.abs().max())
    assert err < GTOL, err                      # (the gradient bar of smoke() / test_layers_gpu: relative to the largest gradient)


def test_embedding_gradients_with_tied_rows():
    """Molecule inputs: h = an embedding of 28 atom types, so neighbourhoods hold tied rows.  Which tied edge gets the max / min
    gradient differs between the kernel (lowest edge id) and autograd (split evenly); the table gradient does not."""
    from gsn_amd import dgn
    b, ei, nf, ef = _molecules()
    d = 70
    table = torch.randn(28, d, device=DEV, dtype=torch.float64)
    codes = torch.from_numpy(b.atom_type).to(DEV)
    t32 = table.float().requires_grad_(True)
    aggs = "mean max min dir1-dx dir1-av"
    y = dgn.dgn_aggregate(t32[codes], ei, aggs, "identity", None, edge_field=ef)
    t64 = table.clone().requires_grad_(True)
    ref = restate(t64[codes], ei, None, ef.double(), aggs, "identity", 1.0)
    w = torch.randn_like(y)
    (y * w).sum().backward()
    (ref * w.double()).sum().backward()
    assert elementwise_ok(t32.grad.double(), t64.grad, GTOL), float((t32.grad.double() - t64.grad).abs().max())


# ------------------------------------------------------------------------------------------------------------------
# (c) layer and DGNNet against the reference
# ------------------------------------------------------------------------------------------------------------------
def _graph(z, key, with_field=True):
    from gsn_amd import dgn, synth
    b = synth.Batch(z[key + "/node_ptr"], np.zeros(len(z[key + "/node_ptr"]), dtype=np.int64), z[key + "/edge_index"])
    return dgn.DGNGraph.from_batch(b, edge_field=z[key + "/ef"] if with_field else None)


@pytest.mark.parametrize("case", [str(c) for c in load("dgn")["layer/cases"]])
def test_layer_matches_reference(case):
    from gsn_amd import dgn
    z = _z()
    train, gn, res, pl = case.startswith("train"), "gn1" in case, "res1" in case, int(case[-1])
    h0 = z["layer/h"]
    d = h0.shape[1]
    layer = dgn.DGNLayer(d, d, 0.0, gn, True, "mean max min dir1-dx dir1-av", "identity", {"log": 1.0}, "simple", res,
                         posttrans_layers=pl).model
    sd = {k[len("layer/%s/sd/" % case):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("layer/%s/sd/" % case)}
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train(train)
    g = _graph(z, "layer")
    assert torch.equal(g.snorm_n.cpu(), torch.from_numpy(z["layer/snorm_n"]))
    h = _t(h0).requires_grad_(True)
    y = layer(g, h, None, g.snorm_n)
    yr = _t(z["layer/%s/y" % case])
    assert elementwise_ok(y.detach(), yr), (case, float((y.detach() - yr).abs().max()))
    (y * _t(z["layer/%s/w" % case])).sum().backward()
    assert elementwise_ok(h.grad, _t(z["layer/%s/grad_h" % case]), GTOL), case
    refs = {k: _t(z["layer/%s/gp/%s" % (case, k)]) for k, _ in layer.named_parameters()}
    for k, p in layer.named_parameters():
        assert float((p.grad - refs[k]).abs().max()) <= GTOL * _grad_scale(refs, k), (case, k)


def _grad_scale(refs, k):
    """The bar's scale for parameter k's gradient: its own largest reference value -- or, where that vanishes in exact arithmetic (the
    bias in front of a train-mode BatchNorm: the normalisation removes it, so both runs hold rounding noise there), the largest
    reference gradient of the module."""
    top = max(float(g.abs().max()) for g in refs.values())
    own = float(refs[k].abs().max())
    return own if own >= 1e-3 * top else top


NET = dict(L=4, hidden_dim=70, out_dim=70, type_net="simple", residual=True, edge_feat=False, readout="mean", in_feat_dropout=0.0,
           dropout=0.0, graph_norm=False, batch_norm=True, aggregators="mean max min dir1-dx dir1-av", scalers="identity", towers=5,
           divide_input_first=False, divide_input_last=True, edge_dim=0, pretrans_layers=1, posttrans_layers=1, pos_enc_dim=0, device="cuda")


@pytest.mark.parametrize("readout", [str(r) for r in load("dgn")["netv/readouts"]])
def test_dgn_net_pos_enc_and_readouts(readout):
    """pos_enc_dim > 0 (ndata['pos_enc'] through embedding_pos_enc) and the 'sum' / 'max' readouts against the reference."""
    from gsn_amd import dgn
    z = _z()
    net = dgn.DGNNet(dict(NET, L=2, hidden_dim=16, out_dim=16, readout=readout, pos_enc_dim=3, avg_d={"log": 1.0}))
    pre = "netv/%s/sd/" % readout
    net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)})
    net = net.to(DEV).train()
    g = _graph(z, "netv")
    g.ndata["pos_enc"] = _t(z["netv/pos_enc"])
    scores = net(g, _t(z["netv/codes"], torch.int64), None, g.snorm_n, None)
    s64 = _t(z["netv/%s/scores64" % readout], torch.float64)
    assert elementwise_ok(scores.detach().double().t(), s64.t()), float((scores.detach().double() - s64).abs().max())
    net.loss(scores, _t(z["netv/labels"])).backward()
    grads = {k: _t(z["netv/%s/gp64/%s" % (readout, k)]) for k, _ in net.named_parameters()}
    assert any(k.startswith("embedding_pos_enc.") for k in grads)
    for k, p in net.named_parameters():
        assert float((p.grad - grads[k]).abs().max()) <= GTOL * _grad_scale(grads, k), k


def test_dgn_net_forward_gradients_and_adam_step():
    from gsn_amd import dgn
    z = _z()
    net = dgn.DGNNet(dict(NET, avg_d={"log": float(z["net/avg_log"])}))
    net.load_state_dict({k[len("net/sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("net/sd/")})
    net = net.to(DEV).train()
    g = _graph(z, "net")
    codes = _t(z["net/codes"], torch.int64)
    scores = net(g, codes, None, g.snorm_n, None)
    s64 = _t(z["net/scores64"], torch.float64)
    assert elementwise_ok(scores.detach().double().t(), s64.t()), float((scores.detach().double() - s64).abs().max())
    loss = net.loss(scores, _t(z["net/labels"]))
    assert abs(float(loss) - float(z["net/loss64"])) <= TOL * abs(float(z["net/loss64"]))
    opt = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=3e-6)
    opt.zero_grad()
    loss.backward()
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    grads = {k: _t(z["net/gp64/%s" % k]) for k, _ in net.named_parameters()}
    for k, p in net.named_parameters():
        assert float((p.grad - grads[k]).abs().max()) <= GTOL * _grad_scale(grads, k), k
    opt.step()
    top = max(float(g.abs().max()) for g in grads.values())
    for k, p in net.named_parameters():
        ref = _t(z["net/step64/%s" % k])
        # Adam's first step is lr * g / (|g| + 1e-8): well conditioned where the gradient is not noise.  Gradients that vanish in exact
        # arithmetic (the bias before a BatchNorm) are rounding noise in both runs; their steps are only bounded by lr.
        sig = grads[k].abs() > 1e-4 * top
        err = (p.detach() - ref).abs()
        assert float(err[sig].max() if sig.any() else 0.0) <= GTOL * (float(before[k].abs().max()) + 0.01), k
        assert float(err.max()) <= 2.0 * 0.01 + 1e-6, k


# ------------------------------------------------------------------------------------------------------------------
# (d) determinism, (e) graph capture, (f) empty batches
# ------------------------------------------------------------------------------------------------------------------
def test_bit_identical_runs():
    from gsn_amd import dgn
    b, ei, nf, ef = _molecules()
    h = torch.randn(b.num_nodes, 70, device=DEV)
    outs = []
    for _ in range(2):
        hh = h.clone().requires_grad_(True)
        y = dgn.dgn_aggregate(hh, ei, BIG_AGGS, "identity amplification", {"log": 1.1}, node_field=nf, edge_field=ef)
        y.backward(torch.ones_like(y))
        outs.append((y.detach().clone(), hh.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_layer_graph_capture_replays_refilled_batch():
    from gsn_amd import dgn, layers, synth
    b1, b2 = synth.zinc_shape_batch(128, seed=1), synth.zinc_shape_batch(128, seed=2)
    E = min(b1.num_edges, b2.num_edges)
    N = max(b1.num_nodes, b2.num_nodes)

    def inputs(b):      # same shapes for both batches: N nodes (the extra ones isolated), the first E edges
        ei = torch.from_numpy(b.edge_index[:, :E]).to(DEV)
        ef = torch.from_numpy(((b.edge_index[0, :E] * 3 + b.edge_index[1, :E]) % 4).astype(np.float32)).to(DEV).unsqueeze(1)
        return ei, torch.cat([ef, -ef], 1)

    torch.manual_seed(0)
    layer = dgn.DGNLayerSimple(70, 70, 0.0, False, True, "mean max min dir1-dx dir1-av".split(), ["identity"], True, None).to(DEV)
    s_ei, s_ef = inputs(b1)
    s_ei, s_ef = s_ei.clone(), s_ef.clone()
    s_h = torch.randn(N, 70, device=DEV, requires_grad=True)
    s_w = torch.randn(N, 70, device=DEV)

    def step():
        g = dgn.DGNGraph(s_ei, N, edata={"eig": s_ef}, snorm_n=torch.ones(N, 1, device=DEV))
        y = layer(g, s_h, None, g.snorm_n)
        gh, = torch.autograd.grad((y * s_w).sum(), [s_h])
        return y.detach(), gh

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(st)
    layers.drop_input_caches()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        y_s, g_s = step()
    layers.drop_input_caches()
    layers.drop_capture_caches()
    ei2, ef2 = inputs(b2)
    h2 = torch.randn(N, 70, device=DEV)
    with torch.no_grad():
        s_ei.copy_(ei2)
        s_ef.copy_(ef2)
        s_h.copy_(h2)
    cg.replay()
    torch.cuda.synchronize()
    g2 = dgn.DGNGraph(ei2, N, edata={"eig": ef2}, snorm_n=torch.ones(N, 1, device=DEV))
    he = h2.clone().requires_grad_(True)
    ye = layer(g2, he, None, g2.snorm_n)
    ge, = torch.autograd.grad((ye * s_w).sum(), [he])
    assert torch.equal(y_s, ye.detach()) and torch.equal(g_s, ge)


def test_empty_batches():
    from gsn_amd import dgn
    aggs = "mean max std dir0-dx dir1-0.1"
    # N = 0
    h = torch.zeros(0, 8, device=DEV, requires_grad=True)
    y = dgn.dgn_aggregate(h, torch.zeros(2, 0, dtype=torch.int64, device=DEV), aggs, "identity amplification", {"log": 1.0},
                          node_field=torch.zeros(0, 2, device=DEV))
    assert y.shape == (0, 2 * 5 * 8)
    y.sum().backward()
    assert h.grad.shape == (0, 8)
    # E = 0: every row zero, every gradient zero (and written: torch.empty underneath)
    h = torch.randn(50, 8, device=DEV, requires_grad=True)
    y = dgn.dgn_aggregate(h, torch.zeros(2, 0, dtype=torch.int64, device=DEV), aggs, "identity amplification", {"log": 1.0},
                          node_field=torch.randn(50, 2, device=DEV))
    assert y.shape == (50, 80) and float(y.abs().max()) == 0.0
    y.backward(torch.randn_like(y))
    assert float(h.grad.abs().max()) == 0.0
    # E = 0 through the layer (BatchNorm over the zero rows' posttrans bias)
    layer = dgn.DGNLayerSimple(8, 8, 0.0, False, True, aggs.split(), ["identity"], True, None).to(DEV)
    g = dgn.DGNGraph(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 50, ndata={"eig": torch.randn(50, 2, device=DEV)})
    out = layer(g, h, None, g.snorm_n)
    assert torch.isfinite(out).all()
