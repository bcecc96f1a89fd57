"""CPU checks of the device-resident loader (gsn_amd/loader.py, csrc/loader.hip): the referee tests/loader_ref.py against a per-graph Python
loop, the epoch plan builder against a naive double loop, the epoch orders, the address arithmetic of gsn_amd/csrc/loader_core.h run on the
host by the stand-alone program tests/loader_harness.cpp (built with the address and undefined-behaviour sanitizers, run as a process), the
refusals of DeviceDataset (decided on the host, in front of the GPU check) and of the entry point, and the no-CPU-fallback error."""
import os
import subprocess

import numpy as np
import pytest
import torch

from gsn_amd.data import Data
from loader_ref import collate_ref, make_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def datasets():
    return {v: make_dataset(11, v) for v in ("A", "B")}


def test_fixture_datasets_hold_their_edge_cases(datasets):
    for v in ("A", "B"):
        gs = datasets[v]
        assert len(gs) == 40 and all(1 <= g.x.shape[0] <= 70 for g in gs)
        assert gs[3].x.shape[0] == 1 and max(g.x.shape[0] for g in gs) == 70
        assert sum(g.edge_index.shape[1] == 0 for g in gs) >= 3 and tuple(gs[19].edge_index.shape) == (2, 0)
        assert gs[11].degrees.shape[0] < gs[11].x.shape[0]
        assert all(int(g.edge_index.max()) < g.x.shape[0] for g in gs if g.edge_index.shape[1])
        assert isinstance(gs[0].graph_size, int) and gs[0].edge_features.dim() == 1
    a, b = datasets["A"][0], datasets["B"][0]
    assert a.x.dtype == torch.int64 and a.x.shape[1] == 1 and a.identifiers.shape[1] == 5 and tuple(a.y.shape) == (1,)
    assert b.x.dtype == torch.float32 and b.x.shape[1] == 5 and b.identifiers.shape == (b.x.shape[0], 3) and tuple(b.y.shape) == (1, 3)
    assert b.coords.dtype == torch.float64 and b.tags.dtype == torch.int32


@pytest.mark.parametrize("variant", ["A", "B"])
def test_referee_against_a_per_graph_loop(datasets, variant):
    graphs = datasets[variant]
    rng = np.random.default_rng(3)
    for idx in ([0], [3], list(range(40)), rng.permutation(40)[:7].tolist(), [19, 7, 3, 11]):
        ref = collate_ref(graphs, idx)
        rows = {k: [] for k, _ in graphs[0]}
        batch, ptr, eptr, offset = [], [0], [0], 0
        for slot, i in enumerate(idx):
            g = graphs[i]
            n = g.x.shape[0]
            for k, v in g:
                if k == "edge_index":
                    rows[k].append([[int(a) + offset for a in v[0]], [int(a) + offset for a in v[1]]])
                elif isinstance(v, (int, float)):
                    rows[k].append(v)
                else:
                    rows[k].extend(v.tolist())
            batch.extend([slot] * n)
            offset += n
            ptr.append(offset)
            eptr.append(eptr[-1] + g.edge_index.shape[1])
        for k, v in graphs[0]:
            got = getattr(ref, k)
            if k == "edge_index":
                want = torch.tensor([sum((r[0] for r in rows[k]), []), sum((r[1] for r in rows[k]), [])], dtype=torch.int64).reshape(2, -1)
            elif isinstance(v, int):
                want = torch.tensor(rows[k], dtype=torch.int64)
            else:
                want = torch.tensor(rows[k], dtype=v.dtype).reshape((-1,) + tuple(v.shape[1:]))
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (k, idx)
        assert ref.batch.tolist() == batch and ref.ptr.tolist() == ptr and ref.edge_ptr.tolist() == eptr and ref.num_graphs == len(idx)
        assert ref.batch.dtype == torch.int64 and ref.ptr.dtype == torch.int64


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("batch_size", [1, 7, 40, 64])
@pytest.mark.parametrize("G", [1, 5, 40])
def test_epoch_plan_against_a_double_loop(G, batch_size, drop_last):
    from gsn_amd.loader import epoch_plan
    rng = np.random.default_rng(100 * G + batch_size)
    C, G_storage = 3, G + 4                                   # (a subset: the order names storage graphs)
    sizes = rng.integers(0, 9, (C, G_storage)).astype(np.int64)
    order = rng.permutation(G_storage)[:G].astype(np.int64)
    plan, totals, n_batches = epoch_plan(sizes, order, batch_size, drop_last)
    assert plan.dtype == np.int64 and plan.shape == (C, G) and plan.flags["C_CONTIGUOUS"]
    assert n_batches == (G // batch_size if drop_last else -(-G // batch_size)) and totals.shape == (C, n_batches)
    for c in range(C):
        for i in range(G):
            lo = i // batch_size * batch_size
            assert plan[c, i] == sum(int(sizes[c, order[j]]) for j in range(lo, i)), (c, i)
        for b in range(n_batches):
            assert totals[c, b] == sum(int(sizes[c, order[j]]) for j in range(b * batch_size, min((b + 1) * batch_size, G))), (c, b)


def test_epoch_orders():
    from gsn_amd.loader import EpochOrder
    G = 40
    seq = EpochOrder(False)
    assert seq.draw(G).tolist() == list(range(G)) and seq.draw(G).dtype == torch.int64
    gen = torch.Generator()
    gen.manual_seed(5)
    sh = EpochOrder(True, gen)
    first = [sh.draw(G) for _ in range(3)]
    for p in first:
        assert p.dtype == torch.int64 and not p.is_cuda and sorted(p.tolist()) == list(range(G))
    assert first[0].tolist() != first[1].tolist() and first[1].tolist() != first[2].tolist()
    gen2 = torch.Generator()
    gen2.manual_seed(5)
    again = EpochOrder(True, gen2)
    assert [again.draw(G).tolist() for _ in range(3)] == [p.tolist() for p in first]
    # generator=None: a private generator seeded from torch.initial_seed(), not the global stream
    torch.manual_seed(123)
    a = EpochOrder(True)
    state = torch.get_rng_state()
    pa = [a.draw(G).tolist() for _ in range(2)]
    assert torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(123)
    b = EpochOrder(True)
    assert [b.draw(G).tolist() for _ in range(2)] == pa and pa[0] != pa[1]


def test_address_arithmetic_on_host_under_sanitizers():
    """csrc/loader_core.h -- pair numbering, segments, destination offsets, the element loops, the edge increment, the pointer writes -- by a
    stand-alone program: every pair and lane of generated datasets byte for byte against a plain concatenation (destinations of exact size,
    so a byte past one is an ASan report), and the int64 arithmetic with offsets beyond 2^32 on a fake base."""
    exe = os.path.join(REPO, "tests", "_build", "loader_harness")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(REPO, "tests", "loader_harness.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("loader harness ok")


def _clone(graphs):
    out = []
    for g in graphs:
        d = Data()
        for k, v in g:
            setattr(d, k, v)
        out.append(d)
    return out


def test_refusals(datasets):
    """Everything DeviceDataset refuses is refused on the host, in front of the GPU check: this runs with or without a GPU."""
    from gsn_amd.loader import GSN_LOADER_MAX_FIELDS, DeviceDataset
    assert GSN_LOADER_MAX_FIELDS == 16
    gs = _clone(datasets["A"][:6])
    gs[4].degrees = gs[4].degrees.double()
    with pytest.raises(TypeError, match=r"'degrees' of graph 4"):
        DeviceDataset(gs)
    gs = _clone(datasets["A"][:6])
    gs[2].identifiers = gs[2].identifiers[:, :4]
    with pytest.raises(ValueError, match=r"'identifiers' of graph 2"):
        DeviceDataset(gs)
    gs = _clone(datasets["A"][:6])
    del gs[5].__dict__["edge_features"]
    with pytest.raises(ValueError, match=r"graph 5 .*'edge_features'"):
        DeviceDataset(gs)
    gs = _clone(datasets["B"][:3])
    for g in gs:
        for j in range(8):
            setattr(g, "extra%d" % j, torch.zeros(1))
    assert len(gs[0].keys) == 17
    with pytest.raises(ValueError, match="16"):
        DeviceDataset(gs)
    gs = _clone(datasets["A"][:6])
    for g in gs:
        g.mask = torch.zeros(g.x.shape[0], dtype=torch.bool)
    with pytest.raises(TypeError, match=r"'mask' of graph 0"):
        DeviceDataset(gs)
    gs = _clone(datasets["A"][:6])
    ei = gs[1].edge_index.clone()
    ei[1, 0] = gs[1].x.shape[0]
    gs[1].edge_index = ei
    with pytest.raises(ValueError, match=r"edge_index of graph 1 .*outside \[0, %d\)" % gs[1].x.shape[0]):
        DeviceDataset(gs)
    gs = _clone(datasets["A"][:6])
    gs[3].graph_size = "one"
    with pytest.raises(TypeError, match=r"'graph_size' of graph 3"):
        DeviceDataset(gs)
    gs = _clone(datasets["A"][:6])
    gs[0].flag = True
    for g in gs[1:]:
        g.flag = False
    with pytest.raises(TypeError, match=r"'flag' of graph 0"):
        DeviceDataset(gs)
    with pytest.raises(ValueError):
        DeviceDataset([])


def test_entry_point_checks_arguments_before_any_launch():
    from gsn_amd import _abi
    _abi.build()
    lib = _abi.lib()
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data

    def table(n, **kw):
        t = (_abi.gsn_loader_field * max(n, 1))()
        for r in t:
            r.src, r.row_ptr, r.dst, r.dst_rows, r.row_bytes, r.elem_bytes = p, p, p, 3, 8, 8
            for k, v in kw.items():
                setattr(r, k, v)
        return t

    call = lib.gsn_loader_collate_hip
    assert call(2, table(2), p, p, 10, 0, 0, p, p, p, None) == 0                          # batch == 0: nothing to do
    assert call(0, None, p, p, 10, 0, 4, p, p, p, None) == 0                              # no fields
    assert call(2, table(2, dst=None, dst_rows=0), p, p, 10, 0, 4, None, None, None, None) == 0      # every destination empty
    assert call(17, table(17), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(2, table(2, elem_bytes=2, row_bytes=2), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(2, table(2, elem_bytes=16, row_bytes=16), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(2, table(2, elem_bytes=8, row_bytes=20), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(2, table(2, dst=None), p, p, 10, 0, 4, p, p, p, None) == -1               # rows without a destination
    assert call(2, table(2, src=None), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(2, table(2, row_ptr=None), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(2, table(2), None, p, 10, 0, 4, p, p, p, None) == -1                      # no order
    assert call(2, table(2), p, None, 10, 0, 4, p, p, p, None) == -1                      # no plan
    assert call(2, table(2), p, p, 10, 8, 4, p, p, p, None) == -1                         # positions past the order
    assert call(2, table(2), p, p, 10, -1, 4, p, p, p, None) == -1
    assert call(2, table(2, kind=5), p, p, 10, 0, 4, p, p, p, None) == -1
    assert call(1, table(1, kind=1, elem_bytes=4, row_bytes=4), p, p, 10, 0, 4, p, p, p, None) == -1      # edge_index is int64
    assert b"gsn_loader_collate_hip" in lib.gsn_last_error()


def test_no_cpu_fallback(datasets):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gsn_amd.loader import DataLoader, DeviceDataset
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceDataset(datasets["A"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DataLoader(datasets["B"], batch_size=4)
