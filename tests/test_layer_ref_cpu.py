"""The float64 layer check of tests/layer_ref.py has teeth: on the tile-boundary batch the fp32 oracle is inside the yardstick's caps,
the float64 restatement that carries the rounding scale equals ``oracle.layer_forward`` in float64, and every seeded defect FAILS the
check that tests/test_layer_f64_gpu.py applies to the kernels.  No GPU.

Detection thresholds (measured by ``measure_thresholds()`` below on the boundary batch, GSN_edge_sparse 28 / 12 / 4, d = 128, relu +
BatchNorm; recorded, not asserted).  A relative perturbation 2^-k of the operand of one Linear stage, smallest power of two still
detected:

    Linear (its operand)     inputs   this check   the earlier bound 1e-5 |ref| + 1e-5 max|ref row|   at 2^-20: max q, share of the earlier bound
    msg_fn.fc.0              exact    2^-18        2^-15                                               10.2   0.062
    msg_fn.fc.1              exact    2^-19        2^-16                                               19.8   0.073
    update_fn.fc.0           exact    2^-19        2^-16                                               23.2   0.078
    update_fn.fc.1           exact    2^-20        2^-15                                               26.7   0.080
    msg_fn.fc.0              real     2^-19        2^-16                                               14.7   0.093
    msg_fn.fc.1              real     2^-19        2^-16                                               14.7   0.098
    update_fn.fc.0           real     2^-19        2^-16                                               26.2   0.082
    update_fn.fc.1           real     2^-19        2^-15                                               26.2   0.081

so the check sees an error 8 to 32 times smaller than the bound of the earlier layer tests did (the fp32 oracle itself sits at max q32
8.8 .. 27.0, rms q32 1.1 .. 3.0 on the cases of this file).
"""
import pytest
import torch

import layer_ref as R

CTOR = dict(d_in=28, d_ef=4, d_id=12, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128,
            d_up=128, d_h=[128], seed=0, activation_name="relu", bn=True, msg_kind="general", flow="source_to_target")


def _base(**over):
    base = dict(d_degree=1, degree_as_tag=False, retain_features=True, seed=0, activation_name="relu", bn=True, msg_kind="general",
                flow="source_to_target", d_msg=128, d_up=128, d_h=[128])
    base.update(over)
    return base


# (class, constructor, d_x, d_id, d_ef, input kind, lead): all four classes, both id scopes, both flows, relu / identity, BatchNorm on / off
CASES = {
    "gsn_e-exact": ("GSN_edge_sparse", CTOR, 28, 12, 4, "exact", 0),
    "gsn_e-real": ("GSN_edge_sparse", CTOR, 28, 12, 4, "real", 0),
    "gsn_e-mixed-lead1": ("GSN_edge_sparse", CTOR, 28, 12, 4, "mixed", 1),
    "gsn_e-exact-lead31-t2s": ("GSN_edge_sparse", dict(CTOR, flow="target_to_source"), 28, 12, 4, "exact", 31),
    "gsn_e-real-identity-bn": ("GSN_edge_sparse", dict(CTOR, activation_name="identity"), 28, 12, 4, "real", 0),
    "gsn_e-exact-relu-nobn": ("GSN_edge_sparse", dict(CTOR, bn=False), 28, 12, 4, "exact", 0),
    "gsn_v-global-real": ("GSN_sparse", _base(d_in=16, d_id=8, id_scope="global"), 16, 8, 0, "real", 0),
    "gsn_v-local-exact": ("GSN_sparse", _base(d_in=28, d_id=16, id_scope="local"), 28, 16, 0, "exact", 0),
    "mpnn_e-real": ("MPNN_edge_sparse", _base(d_in=28, d_ef=4), 28, 0, 4, "real", 31),
    "mpnn-exact-d4": ("MPNN_sparse", _base(d_in=4), 4, 0, 0, "exact", 0),
    "mpnn-pow2-d128": ("MPNN_sparse", _base(d_in=128), 128, 0, 0, "pow2", 0),
    "gsn_e-relu-d128-identity-bn": ("GSN_edge_sparse", _base(d_in=128, d_ef=4, d_id=12, id_scope="local", activation_name="identity"), 128, 12, 4, "relu", 0),
    "gsn_e-exact-d64": ("GSN_edge_sparse", _base(d_in=28, d_ef=4, d_id=12, id_scope="local", d_msg=64, d_up=64, d_h=[64]), 28, 12, 4, "exact", 0),
}

_MADE = {}


def make_case(name):
    """-> dict(cls, ctor, sd, x, ei, ids, ef, y64, sigma, y32): built once per module run and left unchanged"""
    if name not in _MADE:
        cls, ctor, d_x, d_id, d_ef, kind, lead = CASES[name]
        n, ei, _ = R.boundary_batch(5, lead=lead)
        if ctor.get("flow") == "target_to_source":
            ei = ei.flip(0).contiguous()                  # (the prescribed in-degrees belong to the aggregating end)
        _, sd = R.layer_state(cls, ctor, 3)
        x, ids, ef = R.make_inputs(kind, 7, n, ei.shape[1], d_x, d_id, d_ef, ids_per_node=ctor.get("id_scope") == "global")
        y64, sigma = R.reference(cls, ctor, sd, x, ei, ids, ef)
        y32 = R.oracle32(cls, ctor, sd, x, ei, ids, ef)
        _MADE[name] = dict(cls=cls, ctor=ctor, sd=sd, x=x, ei=ei, ids=ids, ef=ef, y64=y64, sigma=sigma, y32=y32, n=n)
    return _MADE[name]


def test_boundary_batch_is_what_it_says():
    n, ei, node_ptr = R.boundary_batch(5)
    assert n == 257 and ei.shape == (2, 1378) and node_ptr.tolist() == [0, 257]
    deg = R.in_degrees(ei, n)
    assert deg.tolist() == R.DEGREES
    assert deg[:16].tolist() == [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 0, 300, 2, 3]
    assert deg[16:56].sum() == 0 and deg[15] > 0 and deg[56] > 0 and deg[-1] == 0
    assert bool((ei[1][1:] < ei[1][:-1]).any())                                       # shuffled
    assert len(set(map(tuple, ei.t().tolist()))) < ei.shape[1]                        # repeated edges occur
    for lead in (1, 31):
        n2, ei2, _ = R.boundary_batch(5, lead=lead)
        assert R.in_degrees(ei2, n2).tolist() == [0] * lead + R.DEGREES
    n4, ei4, _ = R.boundary_batch(5, repeat=4)
    assert n4 == 1028 and R.in_degrees(ei4, n4).tolist() == R.DEGREES * 4
    # the collated form of csrc/layer_g.hip
    n3, ei3, ptr3 = R.boundary_batch(5, per_graph=True)
    sizes = (ptr3[1:] - ptr3[:-1]).tolist()
    assert sizes == [1, 2, 127, 128, 128, 5] and n3 == sum(sizes)
    g_src = torch.searchsorted(ptr3, ei3[0].contiguous(), right=True) - 1
    g_tgt = torch.searchsorted(ptr3, ei3[1].contiguous(), right=True) - 1
    assert torch.equal(g_src, g_tgt)
    eptr = R.edge_ptr_of(ei3, ptr3)
    assert int(eptr[-1]) == ei3.shape[1] and int((eptr[1:] - eptr[:-1]).min()) == 0   # a graph without any edge
    deg3 = R.in_degrees(ei3, n3)
    assert int(deg3.max()) == 129 and {31, 32, 33, 63, 64, 65, 127, 128, 129} <= set(deg3.tolist())


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_oracle_is_inside_the_caps_and_passes(name):
    c = make_case(name)
    mx, rms = R.yardstick(c["y32"], c["y64"], c["sigma"])
    print("%s: fp32 oracle max q32 %.1f rms q32 %.2f" % (name, mx, rms))
    assert R.check(c["y32"], c["y32"], c["y64"], c["sigma"]) == (1.0, 1.0)
    # the restatement that carries sigma is the oracle's layer in float64
    y, _ = R.forward64(c["cls"], c["ctor"], c["sd"], c["x"], c["ei"], c["ids"], c["ef"])
    assert float(((y - c["y64"]).abs() / (c["y64"].abs() + c["y64"].abs().amax(dim=1, keepdim=True))).max()) < 1e-13


def _defects(c):
    deg = R.in_degrees(c["ei"].flip(0) if c["ctor"].get("flow") == "target_to_source" else c["ei"], c["n"])
    node = lambda d: int(torch.nonzero(deg == d)[0])
    out = [("operand", k, 2.0 ** -16) for k in range(4)]
    out += [("drop_edge", node(33)), ("dup_edge", node(64))]
    # the BatchNorm column with the largest |shift| (1e-4 of a shift near zero is below the rounding of the stage itself, and a column
    # whose relu never opens carries no defect at all): a property of the parameters, not of any result
    out += [("bn_shift", p, int(c["sd"][p + ".bn.0.bias"].abs().argmax())) for p in ("msg_fn", "update_fn")]
    return out + [("drop_bias", 5)]


@pytest.mark.parametrize("name", ["gsn_e-exact", "gsn_e-real"])
def test_seeded_defects_fail_the_check(name):
    c = make_case(name)
    for defect in _defects(c):
        y, _ = R.forward64(c["cls"], c["ctor"], c["sd"], c["x"], c["ei"], c["ids"], c["ef"], defect=defect)
        mx, rms = R.quotients(y, c["y64"], c["sigma"])
        print("%s %s: max q %.1f rms q %.2f, old bound used to %.3f" % (name, defect, mx, rms, R.old_bound_ratio(y, c["y32"])))
        assert mx > 0.0, defect                                                      # (the defect changes the result at all)
        assert not R.passes(y.float(), c["y32"], c["y64"], c["sigma"]), defect
        assert not R.passes(y, c["y32"], c["y64"], c["sigma"]), defect


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_sum_given_to_the_node_across_the_tile_edge_fails(kind):
    """node 32's sum given to node 31 -- on the batch with 31 leading isolated nodes, where node 31 (degree 0) ends the first 32-node tile and
    node 32 (degree 1) starts the second; on the batch without leading nodes both sums are empty and the defect changes nothing"""
    n, ei, _ = R.boundary_batch(5, lead=31)
    deg = R.in_degrees(ei, n)
    assert deg[31] == 0 and deg[32] == 1
    _, sd = R.layer_state("GSN_edge_sparse", CTOR, 3)
    x, ids, ef = R.make_inputs(kind, 7, n, ei.shape[1], 28, 12, 4)
    y64, sigma = R.reference("GSN_edge_sparse", CTOR, sd, x, ei, ids, ef)
    y32 = R.oracle32("GSN_edge_sparse", CTOR, sd, x, ei, ids, ef)
    assert R.passes(y32, y32, y64, sigma)
    y, _ = R.forward64("GSN_edge_sparse", CTOR, sd, x, ei, ids, ef, defect=("give_sum", 32, 31))
    assert not R.passes(y, y32, y64, sigma)


def measure_thresholds():
    """the table of the module's docstring"""
    for name in ("gsn_e-exact", "gsn_e-real"):
        c = make_case(name)
        for k in range(4):
            new = old = None
            for p in range(8, 26):
                y, _ = R.forward64(c["cls"], c["ctor"], c["sd"], c["x"], c["ei"], c["ids"], c["ef"], defect=("operand", k, 2.0 ** -p))
                if not R.passes(y, c["y32"], c["y64"], c["sigma"]):
                    new = p
                if R.old_bound_ratio(y, c["y32"]) > 1.0:
                    old = p
            y, _ = R.forward64(c["cls"], c["ctor"], c["sd"], c["x"], c["ei"], c["ids"], c["ef"], defect=("operand", k, 2.0 ** -20))
            print("%s Linear %d: this check detects down to 2^-%s, the earlier bound down to 2^-%s; at 2^-20: max q %.1f, %.3f of the earlier bound"
                  % (name, k, new, old, R.quotients(y, c["y64"], c["sigma"])[0], R.old_bound_ratio(y, c["y32"])))


if __name__ == "__main__":
    measure_thresholds()
