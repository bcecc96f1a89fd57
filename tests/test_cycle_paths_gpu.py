"""The cycle columns' fast path of the counting kernel (count_core.h: cycle_walk; count.hip: the CYC instantiation) against the plan
interpreter it replaces.  The library reads GSN_COUNT_CYCLE once per process, so the same launches run in two child processes
(tests/cycle_paths_child.py), switch on and off, and every output must be bit-equal: int64 identifiers, fp32 encoded rows, fp16 pack
columns, status words -- on ZINC-shaped batches (count_batch and CountLayerStep), pairs beyond 64 vertices, self loops, duplicated and
one-way columns, out-of-range indices, empty graphs and odd graph counts.  Launches outside the rule still match the goldens."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import case_names, count_case

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(path, switch):
    env = dict(os.environ, GSN_COUNT_CYCLE=switch, GSN_CHAIN_TRACE="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "cycle_paths_child.py"), str(path)], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return dict(np.load(str(path))), r.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cycle_paths")
    on, err_on = _child(d / "on.npz", "1")
    off, err_off = _child(d / "off.npz", "0")
    return on, off, err_on, err_off


def test_switch_selects_the_path(runs):
    _, _, err_on, err_off = runs
    assert "cycle walk 1" in err_on and "count_kernel<1,64>" in err_on
    assert "cycle walk 1" not in err_off and "molecule instantiation 1 cycle walk 0" in err_off


def test_every_output_is_bit_equal_between_the_two_paths(runs):
    on, off, _, _ = runs
    assert sorted(on) == sorted(off) and len(on) > 40
    for k in sorted(on):
        a, b = on[k], off[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a, b.view(np.uint8) if b.dtype.kind == "f" else b), k


def test_the_cases_are_what_they_claim(runs):
    """The compared launches really hold the situations they are there for (equal outputs of two paths that both saw nothing prove nothing)."""
    on, _, _, _ = runs
    assert (on["zinc/ids"].max(axis=0) > 0).all() and on["zinc/status"].max() == 0 and len(on["zinc/status"]) == 3001
    assert (on["zinc_perm/ids"][:, [1, 3, 0, 2]] == on["zinc/ids"]).all()
    assert (on["step/ids"] == on["zinc/ids"]).all() and on["step/status"].max() == 0
    assert (on["wide_pairs/ids"].max(axis=0) > 0).all() and on["wide_pairs/status"].max() == 0
    st = on["odd_lot/status"]
    assert len(st) == 2101 and (st == 1).sum() >= 20 and (st == 3).sum() >= 20 and (st == 0).sum() > 1800      # KeyError, bad index
    assert on["odd_lot/ids"].max() >= 5 * 4 * 3 * 2        # K7: 6-cycles through an edge


def _launch_golden(name, fixture):
    from gsn_amd.counting import CountPlan, count_batch
    c = count_case(name, fixture)
    plan = CountPlan(c["patterns"], c["mode"], c["induced"], c["directed_orbits"])
    dev = torch.device("cuda", 0)
    out, st = count_batch(plan, c["node_ptr"], c["edge_ptr"], c["edge_index_local"], ids_are_global=False, device=dev)
    assert np.array_equal(out.cpu().numpy(), c["counts"]), name
    if c["mode"] == "edge" and plan.n_cols == 4 and not c["induced"]:      # the launch shape the rule looks at, with the encoder on
        out2, _, enc = count_batch(plan, c["node_ptr"], c["edge_ptr"], c["edge_index_local"], ids_are_global=False, device=dev, encode=([3] * 4, True))
        assert np.array_equal(out2.cpu().numpy(), c["counts"]), name
        assert np.array_equal(enc.cpu().numpy().reshape(-1, 4, 3).argmax(-1), np.minimum(c["counts"], 2)), name


def test_launches_outside_the_rule_match_the_goldens():
    """Vertex mode, induced plans and clique plans keep the interpreter (and the goldens of the reference); so do the cycle cases of the
    goldens, which the rule takes where the launch is a molecule launch."""
    names = case_names("counts")
    picked = [n for n in names if count_case(n)["mode"] == "vertex"][:3] + [n for n in names if count_case(n)["induced"]][:3] + \
             [n for n in names if count_case(n)["mode"] == "edge" and not count_case(n)["induced"]][:4]
    assert len(picked) >= 6
    for n in picked:
        _launch_golden(n, "counts")
    for n in case_names("counts_cliques")[:4]:
        _launch_golden(n, "counts_cliques")
