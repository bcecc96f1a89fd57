"""gsn_wgrad_hip (csrc/backward.hip): the weight gradient gW += gH^T [X_0 | ... | X_4] of every dense stage that is not on the fp16x3 kernel
(torch.nn.Linear's weight.grad under models_misc.py:52-58), on all eleven instantiations of its three kernels, against float64 -- the cases of
tests/wgrad_cases.py: blocks read through 32-bit and 64-bit row indices (the x_i / x_j blocks of an edge stage), slabs of exactly 16, 32 and 48 rows
and one more, a last slab of one row, a ninth slab, block seams and tile edges inside one tile, the 2 048-workgroup cap; NaN around everything a
call may read and sentinels around gW.  The default kernels run in this process; GSN_WGRAD_PIPE, GSN_WGRAD_WGS and GSN_WGRAD_FP32 are read once
per process, so the other variants run in four child processes (tests/wgrad_child.py), one after another.  Every call's kernel and slab count are
read back from the library's trace line: a case that lands elsewhere fails."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wgrad_cases as wc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
ALL = wc.names()
SHARED = wc.names(default_process=False)          # the cases the child processes run too
_DONE = {}


def _traced(capfd, fn):
    """fn() with GSN_CHAIN_TRACE set; the weight-gradient lines it printed"""
    capfd.readouterr()
    os.environ["GSN_CHAIN_TRACE"] = "1"
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GSN_CHAIN_TRACE", None)
    return wc.routes(capfd.readouterr().err)


def _ratio(gw, ref, bound):
    return ((gw.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


def _evaluated(name, capfd):
    """One case, computed once for all tests: the float64 product, the bar (twice the error of torch's fp32 product on the device, 3e-7 at least: the
    criterion of test_weight_gradient_bf16x6_vs_fp64) and, for the case with its gathered blocks assembled ("plain") and as it is ("gathered"): gW
    from zeros, gW from a random start G0 after one call and after two, the trace lines, the state of the sentinel bands."""
    if name in _DONE:
        return _DONE[name]
    case = wc.to_device(wc.build(name), DEV)
    gh, x = case.gh[:case.m_rows], wc.x_rows(case)
    ref = gh.double().t() @ x.double()
    bound = gh.double().abs().t() @ x.double().abs()
    err32 = _ratio(gh.t() @ x, ref, bound)
    g0 = (torch.randn(ref.shape, generator=torch.Generator().manual_seed(1)).to(DEV).double() * bound / case.m_rows ** 0.5).float()
    ev = dict(ref=ref, bound=bound, err32=err32, tol=max(2.0 * err32, 3e-7), g0=g0, case=case._replace(gh=None, data=None, idx=None), runs={})
    forms = [("plain", wc.assembled(case))] + ([("gathered", case)] if any(i is not None for i in case.idx) else [])
    for tag, c in forms:
        buf, gw = wc.gw_buffer(c, DEV)
        (route,) = _traced(capfd, lambda: wc.launch(c, gw))
        buf1, gw1 = wc.gw_buffer(c, DEV, g0)
        wc.launch(c, gw1)
        once = gw1.clone()
        wc.launch(c, gw1)
        torch.cuda.synchronize()
        ev["runs"][tag] = dict(gw=gw, once=once, twice=gw1, route=route, has_idx=any(i is not None for i in c.idx), n_blocks=len(c.data),
                               guards=wc.guards_intact(buf) and wc.guards_intact(buf1))
    _DONE[name] = ev
    return ev


@pytest.mark.parametrize("name", ALL)
def test_against_float64_no_nan_and_sentinels(name, capfd):
    """max |gW - ref| / (|gH|^T |X|) <= max(2 err32, 3e-7) over every element; a NaN in gW is a read outside the rows given (a padding row, a
    table row no index names, an index entry behind m_rows); the 4 096 floats on each side of gW keep their bits."""
    ev = _evaluated(name, capfd)
    for tag, r in ev["runs"].items():
        assert not torch.isnan(r["gw"]).any(), tag
        err = _ratio(r["gw"], ev["ref"], ev["bound"])
        print("wgrad %s/%s: err %.3g err32 %.3g" % (name, tag, err, ev["err32"]))
        assert err <= ev["tol"], (tag, err, ev["err32"])
        assert r["guards"], tag


@pytest.mark.parametrize("name", ALL)
def test_added_to_not_overwritten(name, capfd):
    """From a start G0 of the product's scale: G0 + ref within the float64 bar plus one fp32 rounding of the sum; a second call into the same buffer
    adds the product once more (the bar again, from what the first call left)."""
    ev = _evaluated(name, capfd)
    for tag, r in ev["runs"].items():
        want = ev["g0"].double() + ev["ref"]
        excess = ((r["once"].double() - want).abs() - (ev["tol"] * ev["bound"] + 2.0 ** -24 * want.abs())).max().item()
        assert excess <= 0, (tag, "first call", excess)
        want = r["once"].double() + ev["ref"]
        excess = ((r["twice"].double() - want).abs() - (ev["tol"] * ev["bound"] + 2.0 ** -24 * want.abs())).max().item()
        assert excess <= 0, (tag, "second call", excess)


@pytest.mark.parametrize("name", ALL)
def test_route_kernel_and_slabs(name, capfd):
    """The trace names the kernel the block list selects, says `gathered` exactly when a row index is present, and reports the slab count the case is
    there for (tests/wgrad_cases.py)."""
    ev = _evaluated(name, capfd)
    spec, case = wc.SPECS[name], ev["case"]
    for tag, r in ev["runs"].items():
        route = r["route"]
        has_idx = r["has_idx"]
        assert has_idx == (tag == "gathered")
        assert route.gathered == has_idx, (tag, route)
        assert (route.m_rows, route.n_out, route.k, route.blocks) == (case.m_rows, case.n_out, wc.k_total(case), len(case.blocks)), (tag, route)
        assert route.kernel == wc.expected_kernel(r["n_blocks"], has_idx), (tag, route)
        assert (route.slabs, route.slab_rows) == spec.slabs, (tag, route)
        assert (route.slabs - 1) * route.slab_rows < case.m_rows <= route.slabs * route.slab_rows


@pytest.mark.parametrize("name", [n for n in ALL if any(kind != "plain" for _, kind, _ in wc.SPECS[n].blocks)])
def test_gathered_equals_assembled_bit_for_bit_on_one_slab(name, capfd):
    """Reading rows through an index and reading the same rows assembled give the same bits where every element has one writer (one slab); several
    slabs add with float atomics in varying order and are compared with float64 only."""
    ev = _evaluated(name, capfd)
    g, p = ev["runs"]["gathered"], ev["runs"]["plain"]
    if g["route"].slabs == 1 and p["route"].slabs == 1:
        assert torch.equal(g["gw"], p["gw"])
        assert torch.equal(g["once"], p["once"]) and torch.equal(g["twice"], p["twice"])
    else:
        assert wc.SPECS[name].slabs[0] > 1


@pytest.mark.parametrize("name", ["rows16_mixed", "rows64_mixed", "tiles_seams"])
def test_the_poison_is_live(name):
    """The cases are what they claim: the same call told of ONE row more -- the first padding row of gH and of the plain blocks, the first index
    entry behind the rows, which names a NaN table row; all valid addresses -- gives NaN in every element, gathered and assembled, and still does
    with that row of gH made finite (every column of X carries its own poison).  So a kernel that let one such row into a product would fail the
    NaN check above."""
    case = wc.to_device(wc.build(name), DEV)
    finite = case.gh.clone()
    finite[case.m_rows] = 1.0
    case = case._replace(m_rows=case.m_rows + 1)
    for c in (case, wc.assembled(case), case._replace(gh=finite), wc.assembled(case._replace(gh=finite))):
        buf, gw = wc.gw_buffer(c, DEV)
        wc.launch(c, gw)
        assert torch.isnan(gw).all() and wc.guards_intact(buf)


def test_arguments():
    """Zero rows: nothing launched, nothing touched, null data pointers are fine.  No blocks, six blocks, a zero width, a null gW, a null gH with
    rows: GSN_E_INVALID, gW untouched."""
    from gsn_amd import _abi
    L, st = _abi.lib(), _abi.current_stream()
    gh, x = torch.randn(40, 8, device=DEV), torch.randn(40, 8, device=DEV)
    gw = torch.full((8, 8), 3.0, device=DEV)

    def blocks(n, data=x.data_ptr(), width=8):
        arr = (_abi.gsn_block * max(n, 1))()
        for b in range(n):
            arr[b].data = data; arr[b].idx = None; arr[b].idx32 = None; arr[b].width = width
        return arr
    assert L.gsn_wgrad_hip(0, 8, None, 1, blocks(1, data=None), gw.data_ptr(), st) == 0
    assert L.gsn_wgrad_hip(0, 8, None, 2, blocks(2, data=None, width=4), gw.data_ptr(), st) == 0
    invalid = -1
    assert L.gsn_wgrad_hip(40, 8, gh.data_ptr(), 0, blocks(0), gw.data_ptr(), st) == invalid
    assert L.gsn_wgrad_hip(40, 8, gh.data_ptr(), 6, blocks(6, width=1), gw.data_ptr(), st) == invalid
    assert L.gsn_wgrad_hip(40, 8, gh.data_ptr(), 1, blocks(1, width=0), gw.data_ptr(), st) == invalid
    assert b"empty" in L.gsn_last_error()
    assert L.gsn_wgrad_hip(40, 8, gh.data_ptr(), 1, blocks(1), None, st) == invalid
    assert L.gsn_wgrad_hip(40, 8, None, 1, blocks(1), gw.data_ptr(), st) == invalid
    assert b"gsn_wgrad_hip" in L.gsn_last_error()
    torch.cuda.synchronize()
    assert bool((gw == 3.0).all())
    assert L.gsn_wgrad_hip(40, 8, gh.data_ptr(), 1, blocks(1), gw.data_ptr(), st) == 0      # (and the same call with everything in place adds)
    torch.cuda.synchronize()
    assert torch.allclose(gw, 3.0 + gh.t() @ x, rtol=1e-5, atol=1e-5)


def test_training_a_general_layer_takes_the_gather_kernel(capfd):
    """A small GSN_edge_sparse general layer in train mode, forward and backward: its edge stage's weight gradient is a `gathered` call on
    wgrad_bf16_pipe_kernel<gather,6> -- the kernel the cases above test is the one training uses."""
    from gsn_amd import layers
    torch.manual_seed(11)
    n, E, d = 300, 1400, 64
    x = torch.randn(n, 24, device=DEV, requires_grad=True)
    ei = torch.randint(0, n, (2, E), device=DEV)
    layer = layers.GSN_edge_sparse(d_in=24, d_ef=4, d_id=6, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=d, d_up=d,
                                   d_h=[d], seed=0, activation_name="relu", bn=True, msg_kind="general", flow="source_to_target").to(DEV).train()
    kw = dict(identifiers=torch.randn(E, 6, device=DEV), degrees=torch.zeros(n, device=DEV), edge_features=torch.randn(E, 4, device=DEV))
    seen = _traced(capfd, lambda: layer(x, ei, **kw).square().sum().backward())
    gathered = [r for r in seen if r.gathered]
    assert gathered and all(r.kernel == "wgrad_bf16_pipe_kernel<gather,6>" and r.m_rows == E for r in gathered), seen
    assert all(r.kernel.startswith("wgrad_bf16_pipe_kernel<") and r.kernel.endswith(",6>") for r in seen), seen
    assert all(torch.isfinite(p.grad).all() for p in layer.parameters())


# ---------------------------------------------------------------------------------------------------------------------
# the variants behind once-per-process switches
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = {"A": dict(GSN_WGRAD_PIPE="0"), "B": dict(GSN_WGRAD_PIPE="4", GSN_WGRAD_WGS="40"), "C": dict(GSN_WGRAD_PIPE="5"), "D": dict(GSN_WGRAD_FP32="1")}
CHILD_TIMEOUT = 60      # seconds per child: interpreter and runtime start-up, then ~90 small launches


def _child(path, switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSN_WGRAD_")}
    env.update(switches, GSN_CHAIN_TRACE="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "wgrad_child.py"), str(path)], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (switches, r.returncode, r.stderr[-4000:])
    seen, key = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("wgrad case "):
            key = line[len("wgrad case "):]
        elif line.startswith("gsn wgrad: M "):
            assert key is not None and key not in seen, line
            (seen[key],) = wc.routes(line)
    return dict(np.load(str(path))), seen


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """the four child processes, one after another; the first that fails or runs out of time raises here and none is started after it"""
    d = tmp_path_factory.mktemp("wgrad")
    return {v: _child(d / ("%s.npz" % v), sw) for v, sw in VARIANTS.items()}


def _child_gw(arrays, key, case):
    buf = torch.from_numpy(arrays[key])
    return buf, buf[wc.GUARD:-wc.GUARD].view(case.n_out, wc.k_total(case))


def _keys(ev, name):
    return ["%s/%s" % (name, tag) for tag in ev["runs"]]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_runs_the_kernels_its_switches_select(variant, children):
    """A: the unpipelined kernels; B and C: depth 4 and 5 for plain rows, while gathered calls keep the one depth-6 gather instantiation; D: the fp32
    kernel for plain rows, the gather kernel for gathered ones.  B asks for 40 workgroups: the 5000-row case runs as 3 slabs of more than 512
    rows (the long-slab path)."""
    arrays, seen = children[variant]
    sw = VARIANTS[variant]
    pipe, fp32 = int(sw.get("GSN_WGRAD_PIPE", "6")), "GSN_WGRAD_FP32" in sw
    assert len(seen) == len(arrays) > len(SHARED)
    for name in SHARED:
        spec = wc.SPECS[name]
        tags = ["plain"] + (["gathered"] if any(kind != "plain" for _, kind, _ in spec.blocks) else [])
        for tag in tags:
            route = seen["%s/%s" % (name, tag)]
            assert route.gathered == (tag == "gathered"), (name, tag, route)
            assert route.kernel == wc.expected_kernel(len(spec.blocks), tag == "gathered", pipe, fp32), (name, tag, route)
            assert (route.m_rows, route.n_out, route.blocks) == (spec.m_rows, spec.n_out, len(spec.blocks)), (name, tag, route)
            if "GSN_WGRAD_WGS" not in sw:
                assert (route.slabs, route.slab_rows) == spec.slabs, (name, tag, route)
            elif name == "middle":
                assert route.slabs == 3 and route.slab_rows > 512 and 2 * route.slab_rows < spec.m_rows <= 3 * route.slab_rows, (tag, route)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_against_float64_no_nan_and_sentinels(variant, children, capfd):
    arrays, _ = children[variant]
    bad = []
    for name in SHARED:
        ev = _evaluated(name, capfd)
        for key in _keys(ev, name):
            buf, gw = _child_gw(arrays, key, ev["case"])
            err = _ratio(gw.to(DEV), ev["ref"], ev["bound"])
            print("wgrad %s %s: err %.3g err32 %.3g" % (variant, key, err, ev["err32"]))
            if torch.isnan(gw).any() or not err <= ev["tol"] or not wc.guards_intact(buf):
                bad.append((key, err, ev["err32"], bool(torch.isnan(gw).any()), wc.guards_intact(buf)))
    assert not bad, bad


@pytest.mark.parametrize("variant", ["A", "B", "C"])
def test_pipelined_and_unpipelined_kernels_give_the_same_bits_on_one_slab(variant, children, capfd):
    """"Same planes, same products, same order: the same bits" (above wgrad_bf16_pipe_kernel): where the default run and the variant's both report one
    slab -- every element has one writer -- the unpipelined kernels and the depth-4 / 5 pipelines equal the default depth-6 kernels bit for bit,
    plain and gathered.  (The fp32 kernel is another arithmetic: float64 only.)"""
    arrays, seen = children[variant]
    compared, bad = 0, []
    for name in SHARED:
        ev = _evaluated(name, capfd)
        for tag, r in ev["runs"].items():
            key = "%s/%s" % (name, tag)
            if r["route"].slabs != 1 or seen[key].slabs != 1:
                continue
            compared += 1
            if not torch.equal(_child_gw(arrays, key, ev["case"])[1], r["gw"].cpu()):
                bad.append(key)
    assert compared >= 44 and not bad, (compared, bad)      # (the row ladder: 11 row counts x (3 block lists assembled + 1 gathered))
