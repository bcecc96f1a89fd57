"""Float64 reference, element-wise rounding scale and tile-boundary batches for the eval-mode `general` layer.

Shared by tests/test_layer_ref_cpu.py (the checker has teeth) and tests/test_layer_f64_gpu.py (every one-launch layer kernel).  Plain
torch on the CPU only: nothing here touches a GPU or the package's library.

The check.  For a result ``got`` of a case, ``q = |got - y64| / sigma`` over ALL elements, where ``y64`` is ``oracle.layer_forward`` on
float64 copies of the parameters and inputs and ``sigma`` is a root-sum-square rounding scale (u = 2^-24) carried through the same graph
in float64:

    Linear            s2_out = s2_in @ (W*W)^T + u^2 ((v*v) @ (W*W)^T + b*b)
    folded BatchNorm  s2 = s2 scale^2 + u^2 ((v^2 + mean^2) scale^2 + shift^2),  scale = gamma / sqrt(var + eps)
    relu / identity   s2 unchanged
    per-node sum      s2[t] = sum over the in-edges e of t of (s2[e] + u^2 m[e]^2)
    inputs            s2 = 0

``sigma`` is a scale, not a bound: it gives every element its own yardstick (a small element of a row is not hidden behind the row's
maximum).  The yardstick itself is the fp32 oracle on the same case: ``q32`` is the same quotient for ``oracle.layer_forward`` in fp32 and

    max q <= FACTOR max q32        rms q <= FACTOR rms q32        FACTOR = 4

FACTOR is derived, not fitted: the fp16x3 scheme of the kernels drops the x_l w_l term, which the header of csrc/layer_fused.hip bounds at
2^-22 |x w| = 4 u, and otherwise accumulates in fp32 like the oracle.  A degenerate case must not widen the test, so every case also
asserts  max q32 <= 32,  rms q32 <= 4  and  sigma > 0 everywhere  (if a case exceeds a cap, its inputs change, never the cap).
"""
import os
import sys

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _REPO not in sys.path:            # (as tests/conftest.py: also when a test module is run as a script)
    sys.path.insert(0, _REPO)

from oracle import oracle

U = 2.0 ** -24
FACTOR = 4.0
CAP_MAX_Q32 = 32.0
CAP_RMS_Q32 = 4.0

PREFIX = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 0, 300, 2, 3]
DEGREES = PREFIX + [0] * 40 + [2] * 200 + [0]          # N = 257, E = 1378
GRAPH_SIZES = (1, 2, 127, 128, 128, 5)


# ------------------------------------------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------------------------------------------
def _graph_degrees(size, gi):
    """in-degrees of one graph of the per-graph batch: the boundary degrees (up to 129, through repeated edges) where the graph has room"""
    if size <= 2:
        return ([0] * size) if gi == 0 else [1, 33][:size]
    if size <= 8:
        return ([2, 0, 1] + [0] * size)[:size]
    lst = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 0, 2, 3] + [0] * 20
    lst = (lst + [2] * size)[:size - 1] + [0]
    return list(np.roll(lst, 7 * gi))                   # (the boundaries land elsewhere in the tiles of every further graph)


def boundary_batch(seed, per_graph=None, lead=0, repeat=1):
    """-> (N, edge_index int64 [2, E], node_ptr int64).  The in-degrees of ``edge_index[1]`` are prescribed: DEGREES (0, 1, 31 .. 129, a hub
    of 300, forty isolated nodes in a row -- the first behind edges, the last in front of edges --, 200 nodes of degree 2, a final isolated
    node), ``repeat`` times, behind ``lead`` isolated nodes (so that every boundary also falls on the other side of a 32-node tile edge).
    Sources are uniform over the batch (repeated edges and self loops occur), the edge order is shuffled.

    ``per_graph`` (True, or a tuple of graph sizes): a collated batch -- sources inside the target's graph, edges grouped by graph and
    shuffled inside it; sizes 1, 2, 127, 128, 128, 5 by default, the first graph without any edge."""
    rng = np.random.default_rng(seed)
    if per_graph:
        sizes = GRAPH_SIZES if per_graph is True else tuple(per_graph)
        node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        cols = []
        for gi, size in enumerate(sizes):
            deg = np.asarray(_graph_degrees(size, gi), dtype=np.int64)
            tgt = np.repeat(np.arange(size, dtype=np.int64), deg)
            src = rng.integers(0, size, len(tgt))
            p = rng.permutation(len(tgt))
            cols.append(np.stack([src[p], tgt[p]]) + node_ptr[gi])
        return int(node_ptr[-1]), torch.from_numpy(np.concatenate(cols, axis=1)), torch.from_numpy(node_ptr)
    deg = np.asarray([0] * lead + DEGREES * repeat, dtype=np.int64)
    n = len(deg)
    tgt = np.repeat(np.arange(n, dtype=np.int64), deg)
    src = rng.integers(0, n, len(tgt))
    p = rng.permutation(len(tgt))
    return n, torch.from_numpy(np.stack([src[p], tgt[p]])), torch.tensor([0, n], dtype=torch.int64)


def edge_ptr_of(edge_index, node_ptr):
    """edge boundaries of a collated batch whose edges are grouped by graph"""
    g = torch.searchsorted(node_ptr, edge_index[1].contiguous(), right=True) - 1
    assert bool((g[1:] >= g[:-1]).all())
    cnt = torch.bincount(g, minlength=len(node_ptr) - 1)
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt, 0)])


def in_degrees(edge_index, n):
    return torch.bincount(edge_index[1], minlength=n)


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
PACK_VALUES = [0.0, 0.0, 0.0, 1.0, -1.0, 0.5, 1.5, 2.0 ** -10]      # the value set of tests/test_pack16_gpu.py: exact in fp16, below 2


def _log_uniform(shape, lo, hi, g):
    mag = torch.exp(torch.rand(shape, generator=g) * (np.log(hi) - np.log(lo)) + np.log(lo))
    return mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def make_inputs(kind, seed, n, n_edges, d_x, d_id=0, d_ef=0, ids_per_node=False):
    """-> (x, ids or None, ef or None), fp32.  kinds:
    exact   one-hot x and ef, identifiers in {0, 1, 2}                       (rows exact in fp16: two plane products in rr / rp)
    binary  one-hot x and ef, identifiers in {0, 1}                          (what integer codes encode to; below 2: a row pack takes it)
    pack    every input from PACK_VALUES                                      (exact and below 2: what a row pack takes)
    real    x rows times 2^randint(-20, 20), per-edge columns 1e-3 .. 30      (every row on the scaled path)
    mixed   `exact` with 30 % of the per-edge rows made inexact               (exact and inexact rows inside one chunk)
    relu    randn.relu() rows                                                 (hidden-layer inputs of the d = 128 kernels)
    pow2    randn rows times 2^randint(-20, 20)"""
    g = torch.Generator().manual_seed(seed)
    n_id = n if ids_per_node else n_edges
    one_hot = lambda rows, d: torch.nn.functional.one_hot(torch.randint(0, d, (rows,), generator=g), d).float()
    if kind in ("exact", "mixed", "binary"):
        x = one_hot(n, d_x)
        ids = torch.randint(0, 2 if kind == "binary" else 3, (n_id, d_id), generator=g).float() if d_id else None
        ef = one_hot(n_edges, d_ef) if d_ef else None
        if kind == "mixed":
            noisy = torch.rand(n_edges, generator=g) < 0.3
            t = ef if (ids is None or ids_per_node) else ids
            assert t is not None, "mixed inputs need a per-edge input"
            t[noisy] += torch.randn(int(noisy.sum()), t.shape[1], generator=g) * 0.01
    elif kind == "pack":
        vals = torch.tensor(PACK_VALUES)
        pick = lambda rows, d: vals[torch.randint(0, len(vals), (rows, d), generator=g)]
        x = pick(n, d_x)
        ids = pick(n_id, d_id) if d_id else None
        ef = pick(n_edges, d_ef) if d_ef else None
    elif kind in ("real", "pow2", "relu"):
        x = torch.randn(n, d_x, generator=g)
        if kind == "relu":
            x = x.relu()
        else:
            x = x * torch.exp2(torch.randint(-20, 21, (n, 1), generator=g).float())
        ids = ef = None
        if d_id:
            ids = _log_uniform((n_id, d_id), 1e-3, 30.0, g) if kind == "real" else torch.randn(n_id, d_id, generator=g).abs()
        if d_ef:
            ef = _log_uniform((n_edges, d_ef), 1e-3, 30.0, g) if kind == "real" else torch.randn(n_edges, d_ef, generator=g)
    else:
        raise KeyError(kind)
    return x, ids, ef


def randomise_bn(sd, seed):
    """running statistics and affine parameters that are not the identity (in place, on a state dict)"""
    g = torch.Generator().manual_seed(seed)
    for k in sorted(sd):
        v = sd[k]
        if k.endswith("running_mean") or (".bn." in k and k.endswith(".bias")):
            v.copy_(torch.rand(v.shape, generator=g) * 0.6 - 0.3)
        elif k.endswith("running_var") or (".bn." in k and k.endswith(".weight")):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    return sd


# ------------------------------------------------------------------------------------------------------------------------------------
# the float64 forward with its rounding scale (and, for the seeded defects, hooks)
# ------------------------------------------------------------------------------------------------------------------------------------
def _mlp64(sd, prefix, v, s2, act, bn, stage0, defect):
    n_fc = len({k.split(".")[-2] for k in sd if k.startswith(prefix + ".fc.") and k.endswith(".weight")})
    u2 = U * U
    for i in range(n_fc):
        W, b = sd["%s.fc.%d.weight" % (prefix, i)], sd["%s.fc.%d.bias" % (prefix, i)]
        if defect and defect[0] == "operand" and defect[1] == stage0 + i:
            v = v * (1.0 + defect[2])
        if defect and defect[0] == "drop_bias" and prefix == "update_fn" and i == n_fc - 1:
            b = b.clone()
            b[defect[1]] = 0.0
        W2 = W * W
        s2 = s2 @ W2.t() + u2 * ((v * v) @ W2.t() + b * b)
        v = v @ W.t() + b
        if i == n_fc - 1:
            break
        if bn:
            mean, var = sd["%s.bn.%d.running_mean" % (prefix, i)], sd["%s.bn.%d.running_var" % (prefix, i)]
            scale = sd["%s.bn.%d.weight" % (prefix, i)] / torch.sqrt(var + 1e-5)
            shift = sd["%s.bn.%d.bias" % (prefix, i)]
            if defect and defect[0] == "bn_shift" and defect[1] == prefix and i == 0:
                shift = shift.clone()
                shift[defect[2]] *= 1.0 + 1e-4
            s2 = s2 * scale * scale + u2 * ((v * v + mean * mean) * scale * scale + shift * shift)
            v = (v - mean) * scale + shift
        if act == "relu":
            v = v.relu()
        elif act != "identity":
            raise NotImplementedError(act)
    return v, s2


def forward64(cls, ctor, sd, x, ei, ids, ef, defect=None):
    """The eval-mode `general` layer in float64 -> (y, s2): values and the variance of the rounding scale, element-wise.

    ``defect`` seeds one fault into the evaluation (None: none):
      ("operand", k, eps)      the operand of Linear k (msg_fn.fc 0, 1, update_fn.fc 0, 1) times 1 + eps
      ("drop_edge", t)         one in-edge of node t left out of its sum
      ("dup_edge", t)          one in-edge of node t added twice
      ("give_sum", a, b)       node a's sum added to node b's, node a left with none
      ("bn_shift", prefix, c)  column c of the first BatchNorm of msg_fn / update_fn: shift off by 1e-4 of its value
      ("drop_bias", c)         the bias of the last Linear dropped for output column c"""
    f = lambda t: None if t is None else t.double()
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x, ids, ef = f(x), f(ids), f(ef)
    x = x.unsqueeze(-1) if x.dim() == 1 else x
    n = x.shape[0]
    select = 0 if ctor.get("flow", "source_to_target") == "target_to_source" else 1
    idx_i, idx_j = ei[select], ei[1 - select]
    parts = [x[idx_i], x[idx_j]]
    if cls.startswith("GSN"):
        parts += [ids] if ctor.get("id_scope", "local") == "local" else [ids[idx_i], ids[idx_j]]
    if "edge" in cls:
        parts.append(ef.unsqueeze(-1) if ef.dim() == 1 else ef)
    row = torch.cat(parts, -1)
    act, bn = ctor["activation_name"], ctor["bn"]
    m, s2 = _mlp64(sd, "msg_fn", row, torch.zeros_like(row), act, bn, 0, defect)
    n_msg_fc = len({k for k in sd if k.startswith("msg_fn.fc.") and k.endswith(".weight")})
    w = torch.ones(len(idx_i), dtype=torch.float64)
    if defect and defect[0] in ("drop_edge", "dup_edge"):
        # (of the node's in-edges the one with the largest message: with rows spanning 2^-20 .. 2^20 a message 2^-30 of its neighbours' is
        #  below the rounding of the node's sum in any arithmetic, and leaving it out is no observable fault)
        mine = torch.nonzero(idx_i == defect[1]).flatten()
        e = int(mine[m[mine].abs().amax(dim=1).argmax()])
        w[e] = 0.0 if defect[0] == "drop_edge" else 2.0
    agg = torch.zeros(n, m.shape[1], dtype=torch.float64).index_add_(0, idx_i, m * w[:, None])
    s2a = torch.zeros(n, m.shape[1], dtype=torch.float64).index_add_(0, idx_i, s2 + U * U * m * m)
    if defect and defect[0] == "give_sum":
        a, b = defect[1], defect[2]
        agg[b] += agg[a]
        agg[a] = 0.0
    return _mlp64(sd, "update_fn", torch.cat((x, agg), -1), torch.cat((torch.zeros_like(x), s2a), -1), act, bn, n_msg_fc, defect)


def reference(cls, ctor, sd, x, ei, ids, ef):
    """-> (y64, sigma): ``oracle.layer_forward`` on float64 copies, and the element-wise rounding scale"""
    f = lambda t: None if t is None else t.double()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    kw = dict(identifiers=f(ids), degrees=None)
    if ef is not None:
        kw["edge_features"] = f(ef)
    y64 = oracle.layer_forward(cls, ctor, sd64, x.double(), ei, training=False, **kw)
    assert y64.dtype == torch.float64
    _, s2 = forward64(cls, ctor, sd, x, ei, ids, ef)
    return y64, torch.sqrt(s2)


def oracle32(cls, ctor, sd, x, ei, ids, ef):
    kw = dict(identifiers=ids, degrees=None)
    if ef is not None:
        kw["edge_features"] = ef
    return oracle.layer_forward(cls, ctor, sd, x, ei, training=False, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------------------------------
def quotients(got, y64, sigma):
    """-> (max q, rms q) of q = |got - y64| / sigma over all elements"""
    q = (got.double() - y64).abs() / sigma
    return float(q.max()), float(torch.sqrt((q * q).mean()))


def yardstick(y32, y64, sigma):
    """(max q32, rms q32) of the fp32 oracle, with the conditions that keep a degenerate case from widening the test"""
    assert bool((sigma > 0).all()) and bool(torch.isfinite(sigma).all()), "sigma must be positive and finite everywhere"
    mx, rms = quotients(y32, y64, sigma)
    assert mx <= CAP_MAX_Q32, "the fp32 oracle itself is at max q32 = %.1f > %g: change the case's inputs" % (mx, CAP_MAX_Q32)
    assert rms <= CAP_RMS_Q32, "the fp32 oracle itself is at rms q32 = %.2f > %g: change the case's inputs" % (rms, CAP_RMS_Q32)
    return mx, rms


def check(got, y32, y64, sigma, factor=FACTOR, what=""):
    """The check of this module's docstring; -> (max q / max q32, rms q / rms q32).  AssertionError with the figures when it fails."""
    mx32, rms32 = yardstick(y32, y64, sigma)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    mx, rms = quotients(got, y64, sigma)
    r = (mx / mx32, rms / rms32)
    msg = "%s: max q %.1f (fp32 oracle %.1f, ratio %.2f), rms q %.2f (fp32 oracle %.2f, ratio %.2f), factor %g" % (what, mx, mx32, r[0], rms, rms32, r[1], factor)
    assert mx <= factor * mx32 and rms <= factor * rms32, msg
    return r


def passes(got, y32, y64, sigma, factor=FACTOR):
    try:
        check(got, y32, y64, sigma, factor)
    except AssertionError:
        return False
    return True


def old_bound_ratio(got, y32):
    """largest |got - ref| / (1e-5 |ref| + 1e-5 max|ref row|) against the fp32 oracle: the bound of the earlier layer tests (> 1 fails it)"""
    ref = y32.double()
    bound = 1e-5 * ref.abs() + 1e-5 * ref.abs().amax(dim=1, keepdim=True)
    return float(((got.double() - ref).abs() / bound).max())


def layer_state(cls, ctor, seed, d_h_up=None):
    """-> (layer, state dict): a freshly seeded eval-mode layer of the package with randomised BatchNorm vectors and fp32 CPU copies of its
    parameters and buffers -- built on the CPU, no kernel runs.  ``d_h_up``: update_fn with hidden widths of its own (the layer classes
    give msg_fn and update_fn one ``d_h``; the kernels do not ask for that, and some of their instantiations need two widths)."""
    from gsn_amd import layers
    torch.manual_seed(seed)
    layer = getattr(layers, cls)(**ctor)
    if d_h_up is not None:
        uf = layer.update_fn
        layer.update_fn = layers.mlp(uf.in_features, uf.out_features, list(d_h_up), ctor["seed"], ctor["activation_name"], ctor["bn"])
    layer.eval()
    sd = randomise_bn({k: v.clone() for k, v in layer.state_dict().items()}, seed + 1)
    layer.load_state_dict(sd)
    return layer, {k: v.clone() for k, v in sd.items()}
