"""CPU checks of the padded loader (gsn_amd.loader.PaddedDataLoader, csrc/loader_padded_core.h): the host arithmetic -- static shape, default
capacities, fit decisions, pad-graph pointers -- against the referee tests/padded_ref.py on the fixture datasets and on hand-made corner
cases; the per-lane routine of the padded collate run on the host by the stand-alone program tests/padded_harness.cpp (built with the address
and undefined-behaviour sanitizers, run as a process); and the argument checks of the two new entry points, which come before any launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from loader_ref import make_dataset
from padded_ref import batches_of, fits_ref, pad_sizes_ref, shape_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sizes(graphs):
    return [int(g.x.shape[0]) for g in graphs], [int(g.edge_index.shape[1]) for g in graphs]


def _check_loader(n, e, B, shuffle, drop_last, node_capacity=None, edge_capacity=None, orders=None, must_fit=True):
    """shape, and per batch of every order the fit decision and the pad pointers, against the referee; returns the fit decisions"""
    from gsn_amd.loader import pad_pointers, padded_fits, padded_shape
    sh = padded_shape(n, e, B, shuffle, drop_last, node_capacity, edge_capacity)
    ref = shape_ref(n, e, B, shuffle, drop_last, node_capacity, edge_capacity)
    got = dict(n_chunk=sh.n_chunk, e_chunk=sh.e_chunk, N_cap=sh.node_capacity, E_cap=sh.edge_capacity, P=sh.pad_slots, G_cap=sh.graph_slots, B=B)
    assert got == ref, (got, ref)
    assert sh.graph_slots == B + sh.pad_slots and sh.pad_slots >= 1
    fits = []
    for order in orders or [None]:
        for idx in batches_of(len(n), B, drop_last, order):
            b, N_r, E_r = len(idx), sum(n[i] for i in idx), sum(e[i] for i in idx)
            want = fits_ref(ref, b, N_r, E_r)
            assert padded_fits(sh, b, N_r, E_r) == want, (idx, got)
            assert want or not must_fit, ("a batch misses the default capacities", idx, got)
            fits.append(want)
            if not want:
                continue
            pads = pad_sizes_ref(ref, b, N_r, E_r)
            pn, pe = pad_pointers(sh, b, N_r, E_r)
            assert pn.dtype == np.int64 and pe.dtype == np.int64 and len(pn) == len(pe) == len(pads) + 1
            assert pn.tolist() == [N_r + sum(p[0] for p in pads[:k]) for k in range(len(pads) + 1)], idx
            assert pe.tolist() == [E_r + sum(p[1] for p in pads[:k]) for k in range(len(pads) + 1)], idx
            assert pn[-1] == ref["N_cap"] and pe[-1] == ref["E_cap"]
            assert all(1 <= p[0] <= ref["n_chunk"] and 0 <= p[1] <= ref["e_chunk"] for p in pads)
    return fits


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("B", [1, 4, 7, 40, 64])
def test_shape_and_pad_pointers_on_the_fixture_datasets(variant, B):
    n, e = _sizes(make_dataset(11, variant))
    rng = np.random.default_rng(B)
    for drop_last in (False, True):
        _check_loader(n, e, B, False, drop_last)
        _check_loader(n, e, B, True, drop_last, orders=[rng.permutation(len(n)).tolist() for _ in range(5)])
    # a subset, as a split of the dataset is
    sub = rng.permutation(len(n))[:11].tolist()
    _check_loader([n[i] for i in sub], [e[i] for i in sub], B, False, False)


def test_corner_cases():
    rng = np.random.default_rng(0)
    # last batch of one graph; G < B; a single graph
    _check_loader([3, 5, 2, 7, 4], [4, 8, 0, 12, 6], 4, False, False)
    _check_loader([3, 5, 2], [4, 8, 0], 8, False, False)
    _check_loader([3, 5, 2], [4, 8, 0], 8, True, False, orders=[[2, 0, 1]])
    _check_loader([6], [10], 1, False, False)
    _check_loader([6], [10], 3, True, True, orders=[[0]])
    # every graph a single vertex (n_chunk = 2: a pad graph may still take a second vertex)
    _check_loader([1] * 9, [0, 2, 0, 1, 0, 0, 3, 0, 1], 4, False, False)
    _check_loader([1] * 9, [0] * 9, 4, True, False, orders=[rng.permutation(9).tolist() for _ in range(3)])
    # an edgeless dataset: no edge capacity, e_chunk = 1
    sh = _check_loader([2, 7, 1, 4, 4, 3], [0] * 6, 4, False, False)
    assert all(sh)
    # many tiny graphs with many edges each: the pad slots are set by the edge capacity
    _check_loader([1, 2, 1, 2] * 5, [9, 8, 9, 7] * 5, 5, True, False, orders=[rng.permutation(20).tolist() for _ in range(3)])
    # random datasets, sequential and shuffled
    for trial in range(40):
        G, B = int(rng.integers(1, 30)), int(rng.integers(1, 12))
        n = rng.integers(1, 1 + int(rng.integers(1, 20)), G).tolist()
        e = (rng.integers(0, 1 + int(rng.integers(0, 30)), G)).tolist()
        _check_loader(n, e, B, False, bool(trial % 2))
        _check_loader(n, e, B, True, bool(trial % 2), orders=[rng.permutation(G).tolist() for _ in range(3)])


def test_explicit_capacities_missed_by_exactly_one_row():
    n, e, B = [3, 5, 2, 7, 4, 6, 1, 2], [4, 8, 0, 12, 6, 2, 0, 2], 4           # batches: 17 / 24 and 13 / 10
    from gsn_amd.loader import padded_shape
    # the first batch needs N_r + S <= N_cap with S = P: find the node capacity it just fits, then take one away
    for N_cap in range(18, 40):
        sh = padded_shape(n, e, B, node_capacity=N_cap, edge_capacity=24)
        if 17 + sh.pad_slots <= N_cap:
            break
    assert _check_loader(n, e, B, False, False, node_capacity=N_cap, edge_capacity=24, must_fit=False) == [True, True]
    assert _check_loader(n, e, B, False, False, node_capacity=N_cap - 1, edge_capacity=24, must_fit=False) == [False, True]
    assert _check_loader(n, e, B, False, False, node_capacity=N_cap, edge_capacity=23, must_fit=False) == [False, True]
    assert _check_loader(n, e, B, False, False, node_capacity=N_cap, edge_capacity=9, must_fit=False) == [False, False]
    assert _check_loader(n, e, B, False, False, node_capacity=N_cap, edge_capacity=10, must_fit=False) == [False, True]
    with pytest.raises(ValueError):
        padded_shape(n, e, B, node_capacity=0)
    with pytest.raises(ValueError):
        padded_shape(n, e, B, edge_capacity=-1)


def test_padded_routine_on_host_under_sanitizers():
    """csrc/loader_padded_core.h by a stand-alone program: every (field, slot) pair and lane into destinations of exactly the capacities,
    poisoned with 0xA5 (and 0x5A), byte for byte against a plain concatenation plus the pad rule; exactly one writer per byte; the
    closed-form starts and the fit rule at their edges and with offsets beyond 2^32."""
    exe = os.path.join(REPO, "tests", "_build", "padded_harness")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(REPO, "tests", "padded_harness.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("padded harness ok")


def test_entry_points_check_arguments_before_any_launch():
    from gsn_amd import _abi
    _abi.build()
    lib = _abi.lib()
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    flags = [1, 0, 2, 4]                       # x, a per-vertex field, a per-edge field, a per-graph field

    def table(**kw):
        t = (_abi.gsn_loader_field * 4)()
        for r, fl in zip(t, flags):
            r.src, r.row_ptr, r.dst, r.row_bytes, r.elem_bytes, r.flags = p, p, p, 8, 8, fl
            r.dst_rows = {1: 19, 0: 19, 2: 15, 4: 7}[fl]
            for k, v in kw.items():
                setattr(r, k, v)
        return t

    def pad(**kw):
        q = dict(n_real=3, graph_slots=7, n_real_nodes=10, n_real_edges=12, node_capacity=19, edge_capacity=15, n_chunk=4, e_chunk=6)
        q.update(kw)
        return _abi.gsn_loader_pad(**q)

    fill = (ctypes.c_uint64 * 4)()
    call = lib.gsn_loader_collate_padded_hip
    bad = [
        (4, table(), fill, p, p, 10, 0, pad(node_capacity=13), p, p, p, p),                   # a pad slot without a vertex
        (4, table(), fill, p, p, 10, 0, pad(edge_capacity=11), p, p, p, p),                   # real edge columns past the capacity
        (4, table(), fill, p, p, 10, 0, pad(n_real=7), p, p, p, p),                           # no pad slot
        (4, table(), fill, p, p, 10, 0, pad(n_real=0), p, p, p, p),
        (4, table(), fill, p, p, 10, 0, pad(n_chunk=1), p, p, p, p),
        (4, table(), fill, p, p, 10, 8, pad(), p, p, p, p),                                   # positions past the order
        (4, table(dst_rows=19), fill, p, p, 10, 0, pad(), p, p, p, p),                        # a field whose rows are not its capacity
        (4, table(elem_bytes=2, row_bytes=2), fill, p, p, 10, 0, pad(), p, p, p, p),
        (4, table(dst=None), fill, p, p, 10, 0, pad(), p, p, p, p),
        (4, table(), None, p, p, 10, 0, pad(), p, p, p, p),                                   # no fill words
        (4, table(), fill, None, p, 10, 0, pad(), p, p, p, p),                                # no order
        (4, table(), fill, p, p, 10, 0, pad(), p, None, p, p),                                # no node pointer
        (4, table(), fill, p, p, 10, 0, None, p, p, p, p),
        (17, table(), fill, p, p, 10, 0, pad(), p, p, p, p),
        (0, table(), fill, p, p, 10, 0, pad(), p, p, p, p),
    ]
    for args in bad:
        assert call(*args, None) == -1, args
    two_x = table()
    two_x[1].flags = 1
    assert call(4, two_x, fill, p, p, 10, 0, pad(), p, p, p, p, None) == -1
    assert b"gsn_loader_collate_padded_hip" in lib.gsn_last_error()
    acc = lib.gsn_eval_accumulate_counted_hip
    assert acc(1, 1, 5, 1, 1, p, p, None, p, p, None, None, 0, None, None, 0, None) == -1      # no n_valid
    assert b"gsn_eval_accumulate_counted_hip" in lib.gsn_last_error()
    assert acc(9, 0, 5, 1, 1, p, p, p, p, p, None, None, 0, None, None, 0, None) == -1         # unknown loss kind
    assert acc(1, 3, 5, 1, 1, p, p, p, p, p, None, None, 0, None, None, 0, None) == -1         # accuracy without integer targets
    assert acc(1, 1, 0, 1, 1, p, p, p, p, p, None, None, 0, None, None, 0, None) == 0          # no rows: nothing to do
