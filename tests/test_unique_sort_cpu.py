"""CPU checks of the full-range recoding (gsn_unique_sort_hip / gsn_lookup_codes_hip): the scratch formula and the argument checks of the
entry points, which need no GPU, and the sorting network, compaction and searches of gsn_amd/csrc/unique_sort_core.h run on the host by the
test-only harness tests/unique_sort_harness.cpp against np.unique / np.searchsorted."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P = ctypes.POINTER(ctypes.c_int64)
TILE = 4096            # US_TILE of unique_sort_core.h
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libunique_sort_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "unique_sort_harness.cpp")])
    h = ctypes.CDLL(so)
    h.harness_unique_sort.restype = ctypes.c_int64
    h.harness_lookup.restype = ctypes.c_int64
    return h


def test_scratch_bytes_monotone_and_zero_for_empty_shapes(lib):
    f = lib.gsn_unique_sort_scratch_bytes
    assert f(0, 0) == 0 and f(0, 5) == 0 and f(7, 0) == 0 and f(-1, 3) == 0
    ms = [1, 2, 63, 1023, 1024, 1025, 4096, 4097, 300001, 3000001, 1 << 31]
    cs = [1, 2, 3, 7, 64]
    for c in cs:
        got = [f(m, c) for m in ms]
        assert all(a <= b for a, b in zip(got, got[1:])), (c, got)
        assert all(g >= 8 * m * c for g, m in zip(got, ms))
    for m in ms:
        got = [f(m, c) for c in cs]
        assert all(a <= b for a, b in zip(got, got[1:])), (m, got)
    # linear in M: 8 C (1 + 1/1024) bytes per row and two roundings to 256 bytes
    assert f(3000001, 4) <= 3000001 * 4 * 8 * (1 + 1 / 1024) + 8 * 4 + 512


def test_entry_points_check_arguments_before_any_launch(lib):
    """Empty shapes launch nothing and succeed; null pointers with a non-empty shape, a short scratch and an unknown mode are refused -- all
    decided on the host, so this runs without a GPU."""
    from gsn_amd import _abi
    assert lib.gsn_unique_sort_hip(0, 3, None, None, None, None, None, 0, None) == 0
    assert lib.gsn_unique_sort_hip(5, 0, None, None, None, None, None, 0, None) == 0
    assert lib.gsn_unique_sort_hip(5, 2, None, None, None, None, None, 0, None) == -1
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    assert lib.gsn_unique_sort_hip(4, 2, p, p, p, p, p, 8, None) == -4            # GSN_E_NOSPACE
    assert lib.gsn_lookup_codes_hip(0, 3, None, None, None, 0, None, None, None, None) == 0
    assert lib.gsn_lookup_codes_hip(3, 0, None, None, None, 1, None, None, None, None) == 0
    assert lib.gsn_lookup_codes_hip(3, 2, None, None, None, 0, None, None, None, None) == -1
    assert lib.gsn_lookup_codes_hip(3, 2, p, p, p, 7, p, p, p, None) == -1
    assert lib.gsn_lookup_codes_hip(3, 2, p, p, p, 0, p, None, None, None) == -1   # strict needs the status words
    assert issubclass(_abi.GsnError, RuntimeError)


def _columns(m, rng):
    yield "equal", np.full(m, 17, dtype=np.int64)
    yield "permutation", rng.permutation(m).astype(np.int64) - m // 2
    yield "three", rng.choice(np.array([-9, 4, 1 << 50], dtype=np.int64), size=m)
    yield "extremes", rng.choice(np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64), size=m)
    yield "high_bits", rng.integers(0, 1000, size=m).astype(np.int64) << 33
    yield "random", rng.integers(I64_MIN, I64_MAX, size=m, dtype=np.int64, endpoint=True)


@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 1023, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE - 5, 5 * TILE + 77,
                               16 * TILE, 17 * TILE + 3])
def test_network_and_compaction_on_host(harness, m):
    rng = np.random.default_rng(m)
    for name, col in _columns(m, rng):
        col = np.ascontiguousarray(col)
        uniq = np.zeros(max(m, 1), dtype=np.int64)
        codes = np.zeros(max(m, 1), dtype=np.int64)
        launches = ctypes.c_int(0)
        nd = harness.harness_unique_sort(ctypes.c_int64(m), col.ctypes.data_as(I64P), uniq.ctypes.data_as(I64P), codes.ctypes.data_as(I64P),
                                         ctypes.byref(launches))
        u, inv = np.unique(col, return_inverse=True)
        assert nd == len(u), (name, m)
        assert np.array_equal(uniq[:nd], u), (name, m)
        assert np.array_equal(codes[:m], inv), (name, m)
        # one tile sort, then per stage k beyond the tile: a flip, k - 13 whole-column steps, a tile merge
        want, k = (1 if m else 0), 13
        while m and (1 << (k - 1)) < m:
            want, k = want + (k - 12) + 1, k + 1
        assert launches.value == want, (m, launches.value, want)


def test_lookup_modes_on_host(harness):
    u = np.array([I64_MIN, -5, 0, 3, 1 << 40, I64_MAX], dtype=np.int64)
    v = np.array([I64_MIN, I64_MIN + 1, -6, -5, -1, 0, 1, 3, 4, 1 << 40, (1 << 40) + 1, I64_MAX - 1, I64_MAX], dtype=np.int64)
    codes = np.zeros(len(v), dtype=np.int64)
    for uu in (u, u[1:-1], u[:1], u[:0]):
        uu = np.ascontiguousarray(uu)
        bad = harness.harness_lookup(ctypes.c_int64(len(v)), v.ctypes.data_as(I64P), ctypes.c_int64(len(uu)), uu.ctypes.data_as(I64P), 0,
                                     codes.ctypes.data_as(I64P))
        pos = np.searchsorted(uu, v, side="right") - 1
        hit = (pos >= 0) & (uu[np.clip(pos, 0, max(len(uu) - 1, 0))] == v if len(uu) else np.zeros(len(v), bool))
        assert np.array_equal(codes, np.where(hit, pos, -1)) and bad == int((~hit).sum())
        harness.harness_lookup(ctypes.c_int64(len(v)), v.ctypes.data_as(I64P), ctypes.c_int64(len(uu)), uu.ctypes.data_as(I64P), 1,
                               codes.ctypes.data_as(I64P))
        assert np.array_equal(codes, np.clip(pos, 0, None))
