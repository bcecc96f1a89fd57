"""bench.py as it is run for a headline figure: a plain run prints one result line for exactly the steps asked for, and
--dump-outputs writes what the last timed step computed -- the same arrays from two runs with the same arguments, the identifiers
equal to the oracle's counts and the layer rows within the bench's own tolerance of the oracle's layer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = 4096          # more rows than bench.DUMP_ROWS in both outputs: the seeded sample is exercised


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--graphs", str(GRAPHS)]
                       + list(extra), cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import networkx as nx
    import bench
    from gsn_amd import layers
    from oracle import oracle
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _bench("--dump-outputs", a)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "graphs/s" and d["higher_is_better"] is True
    assert d["metric"].startswith("graphs/sec") and d["dtype"]
    assert abs(d["value"] - GRAPHS / (d["ms_per_step"] * 1e-3)) <= 1e-2 * d["value"]      # (ms_per_step: 4 decimals)
    for k in ("roofline", "checked", "cpu_baseline"):
        assert k not in d, k                                  # (--full only)
    _bench("--dump-outputs", b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == sorted("%s%s.npy" % (o, s) for o in ("identifiers", "layer_rows") for s in ("", "_rows", "_colsum"))
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    assert sum(v.nbytes for v in got.values()) <= 64 * 2 ** 20
    for n in names:
        v, w = got[n[:-4]], np.load(os.path.join(b, n))
        assert v.dtype in (np.float32, np.float64), n
        if n.startswith("layer_rows") and not n.endswith("_rows.npy"):
            np.testing.assert_allclose(v, w, rtol=1e-6, atol=1e-6 * float(np.abs(v).max()), err_msg=n)
        else:
            np.testing.assert_array_equal(v, w, err_msg=n)
    assert got["identifiers"].shape == (bench.DUMP_ROWS, 4) and got["layer_rows"].shape == (bench.DUMP_ROWS, 128)

    # the dumped arrays are the timed step's outputs: against the oracle on the same (seeded) batch
    bt = bench.make_batch(GRAPHS, seed=1000)
    pats = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
    local = bt.edge_index - np.repeat(bt.node_ptr[:-1], np.diff(bt.edge_ptr))[None, :]
    ref = oracle.counts2ids("edge", False, bt.node_ptr, bt.edge_ptr, local, pats)
    erows = got["identifiers_rows"].astype(np.int64)
    assert np.array_equal(got["identifiers"], ref[erows].astype(np.float64))
    assert np.array_equal(got["identifiers_colsum"], ref.sum(0).astype(np.float64))
    torch.manual_seed(0)
    layer = layers.GSN_edge_sparse(**bench.CTOR).eval()
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    x = torch.nn.functional.one_hot(torch.from_numpy(bt.atom_type), 28).float()
    ef = torch.nn.functional.one_hot(torch.from_numpy(bt.bond_type), 4).float()
    idf = torch.nn.functional.one_hot(torch.from_numpy(ref).clamp(max=2), 3).reshape(ref.shape[0], 12).float()
    with torch.no_grad():
        yref = oracle.layer_forward("GSN_edge_sparse", bench.CTOR, sd, x, torch.from_numpy(bt.edge_index), identifiers=idf, degrees=None,
                                    edge_features=ef).numpy()
    nrows = got["layer_rows_rows"].astype(np.int64)
    yr = yref[nrows]
    floor = 1e-5 * np.abs(yr).max(axis=1, keepdims=True)
    assert (np.abs(got["layer_rows"] - yr) <= 1e-5 * np.abs(yr) + floor).all()
    np.testing.assert_allclose(got["layer_rows_colsum"], yref.astype(np.float64).sum(0), rtol=1e-4, atol=1e-4 * np.abs(yref).sum(0).max())
