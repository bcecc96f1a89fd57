"""The row helpers of the cycle launch's output loop (gsn_amd/csrc/count_core.h: cyc_row_has_direct, cyc_row_store, cyc_row_mask) on the host
through tests/cycle_rows_harness.cpp.  A staged cell of 0xffff means that the count (65 535 or more) was written to memory from inside the
walk: the output loop must leave that cell alone and still write the others.  No cycle launch can produce it (at most K11 fits a workgroup:
3 024 six-cycles through an edge), so the arm is checked here and not on the GPU."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7
EDGE = [0, 1, 2, 3, 254, 255, 256, 0x7fff, 0x8000, 0xfffe, 0xffff]      # cells around every class count, the sign bit of a halfword, the mark


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libcycle_rows_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "cycle_rows_harness.cpp")])
    lib = ctypes.CDLL(so)
    lib.cycle_rows_mask.restype = ctypes.c_uint32
    return lib


def _rows():
    rng = np.random.default_rng(0)
    rows = list(itertools.product(EDGE, repeat=2))
    rows = [[a, b, a, b] for a, b in rows] + [[b, a, a, b] for a, b in rows] + rng.integers(0, 0x10000, (200, 4)).tolist()
    rows += [[0xffff] * 4, [0] * 4, [0xffff, 0, 0, 0], [0, 0, 0, 0xffff], [0xfffe, 0x7fff, 0x8000, 0x0001], [0x8000, 0x8000, 0x8000, 0x8000]]
    return rows


def _store(harness, cells, wide):
    buf = np.full(8, SENTINEL, dtype=np.int64)
    row = buf[(-(buf.ctypes.data // 8)) % 2:][:4]       # the first 16-byte aligned int64 of the buffer
    assert row.ctypes.data % 16 == 0
    if not wide:
        row = buf[(1 - (buf.ctypes.data // 8)) % 2:][:4]
        assert row.ctypes.data % 16 == 8
    lo, hi = cells[0] | (cells[1] << 16), cells[2] | (cells[3] << 16)
    harness.cycle_rows_store(row.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_uint32(lo), ctypes.c_uint32(hi), int(wide))
    return row.copy(), lo, hi


@pytest.mark.parametrize("wide", [True, False])
def test_a_marked_cell_is_left_alone_and_every_other_cell_is_written(harness, wide):
    for cells in _rows():
        row, lo, hi = _store(harness, cells, wide)
        assert harness.cycle_rows_has_direct(ctypes.c_uint32(lo), ctypes.c_uint32(hi)) == int(0xffff in cells)
        assert row.tolist() == [SENTINEL if c == 0xffff else c for c in cells]


@pytest.mark.parametrize("classes", [[3, 3, 3, 3], [2, 3, 2, 4], [1, 1, 1, 1], [4, 4, 4, 4], [13, 1, 1, 1]])
@pytest.mark.parametrize("clamp", [True, False])
def test_mask_is_the_one_hot_of_the_class_as_bits(harness, classes, clamp):
    """A count of 65 535 and more (the mark) is beyond every class count: the last class when clamped, no bit otherwise.  Class counts of
    <= 16 columns together: what the launcher admits for a mask."""
    ncls_w = sum(n << (8 * c) for c, n in enumerate(classes))
    for cells in _rows():
        lo, hi = cells[0] | (cells[1] << 16), cells[2] | (cells[3] << 16)
        want, first = 0, 0
        for c, n in enumerate(classes):
            cls = min(cells[c], n - 1) if clamp else cells[c]
            if cls < n:
                want |= 1 << (first + cls)
            first += n
        assert harness.cycle_rows_mask(ctypes.c_uint32(lo), ctypes.c_uint32(hi), ctypes.c_uint32(ncls_w), int(clamp)) == want
