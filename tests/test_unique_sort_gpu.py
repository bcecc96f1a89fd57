"""Full-range dataset recoding on the device: gsn_unique_sort_hip (``unique_codes(wide="sort" / "auto")``), the fitted lookup
gsn_lookup_codes_hip (``one_hot_unique.transform``, ``lookup_codes``) and the refusal that stays the default.  The reference is
``np.unique(col, return_inverse=True)`` / ``np.searchsorted`` on the CPU, exact equality everywhere."""
import numpy as np
import pytest
import torch

from gsn_amd import _abi
from gsn_amd import data as gdata
from gsn_amd import encoding

pytestmark = pytest.mark.gpu

TILE = 4096            # US_TILE of gsn_amd/csrc/unique_sort_core.h: keys sorted in one LDS tile; beyond it the whole-column steps start
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
SHAPES = [(1, 1), (2, 1), (63, 2), (64, 2), (65, 2), (TILE - 1, 1), (TILE, 1), (TILE + 1, 7), (2 * TILE + 1, 2), (300001, 3)]
KINDS = ["equal", "permutation", "three", "powers", "extremes", "high_low", "low_high", "table_generator"]


def _table_generator(shape):
    """the generator of test_encoding_gpu.py::test_unique_codes_random: inputs both paths accept"""
    rng = np.random.default_rng(shape[0])
    vals = rng.integers(-5, [3 + 40 * c * c for c in range(shape[1])], size=shape)
    vals[:, 0] = rng.integers(0, 3000, size=shape[0]) * 7 - 1000
    return vals


def _values(kind, shape):
    M, C = shape
    rng = np.random.default_rng(1000 * M + C)
    if kind == "equal":
        return np.tile(np.arange(C, dtype=np.int64) * 3 - 1, (M, 1))
    if kind == "permutation":
        return np.stack([rng.permutation(M).astype(np.int64) * (c + 1) - c * M for c in range(C)], 1)
    if kind == "three":
        return rng.choice(np.array([-7, 5, 1 << 45], dtype=np.int64), size=shape)
    if kind == "powers":
        return rng.choice(np.array([0, 1, 2 ** 40, 2 ** 62], dtype=np.int64), size=shape)
    if kind == "extremes":
        v = rng.integers(-3, 3, size=shape).astype(np.int64)
        v[:, 0] = rng.choice(np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64), size=M)
        if M >= 4:
            v[:4, 0] = [I64_MAX, 0, I64_MIN, -1]
        return v
    if kind in ("high_low", "low_high"):
        high = lambda: rng.integers(-500, 500, size=M).astype(np.int64) << 33                      # noqa: E731
        low = lambda: (np.int64(0x1234567800) << 8) + rng.integers(0, 256, size=M).astype(np.int64)   # noqa: E731
        first = 0 if kind == "high_low" else 1
        return np.stack([high() if (c + first) % 2 == 0 else low() for c in range(C)], 1)
    return _table_generator(shape).astype(np.int64)


def _check_against_numpy(vals, codes, d, uniques):
    assert codes.dtype == torch.int64 and tuple(codes.shape) == vals.shape and len(d) == len(uniques) == vals.shape[1]
    for c in range(vals.shape[1]):
        u, inv = np.unique(vals[:, c], return_inverse=True)
        assert d[c] == len(u), c
        assert uniques[c].dtype == torch.int64 and np.array_equal(uniques[c].numpy(), u), c
        assert np.array_equal(codes[:, c].numpy(), inv), c


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sort_path_equals_numpy(shape, kind):
    vals = _values(kind, shape)
    codes, d, uniques = encoding.unique_codes(torch.from_numpy(vals), wide="sort", return_uniques=True)
    _check_against_numpy(vals, codes, d, uniques)
    if kind == "table_generator":
        # both paths on the same inputs: byte for byte, uniques from the table path included
        codes_t, d_t, uniques_t = encoding.unique_codes(torch.from_numpy(vals), return_uniques=True)
        assert d_t == d and codes_t.numpy().tobytes() == codes.numpy().tobytes()
        assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(uniques_t, uniques))
        codes_p, d_p = encoding.unique_codes(torch.from_numpy(vals))
        assert d_p == d and torch.equal(codes_p, codes)


def test_sort_path_is_deterministic():
    vals = _values("permutation", (300001, 3))
    vals[0:300000:3] = vals[1:300000:3]                   # repeated values as well
    runs = [encoding.unique_codes(torch.from_numpy(vals), wide="sort", return_uniques=True) for _ in range(2)]
    (c0, d0, u0), (c1, d1, u1) = runs
    assert d0 == d1 and c0.numpy().tobytes() == c1.numpy().tobytes()
    assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(u0, u1))


def test_refusal_is_the_default_and_lifted_by_auto():
    wide = torch.tensor([[0], [1 << 40]])
    with pytest.raises(NotImplementedError):
        encoding.unique_codes(wide)
    with pytest.raises(NotImplementedError):
        encoding.unique_codes(wide, wide="refuse")
    with pytest.raises(ValueError):
        encoding.unique_codes(wide, wide="yes")
    codes, d = encoding.unique_codes(wide, wide="auto")
    assert codes.tolist() == [[0], [1]] and d == [2]
    codes, d, u = encoding.unique_codes(wide, wide="auto", return_uniques=True)
    assert codes.tolist() == [[0], [1]] and d == [2] and u[0].tolist() == [0, 1 << 40]
    # inside the table's range "auto" is the table path: the same result as the default
    small = torch.tensor([[3, -1], [0, -1], [3, 7]])
    a, b = encoding.unique_codes(small, wide="auto", return_uniques=True), encoding.unique_codes(small)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] == [2, 2] and [x.tolist() for x in a[2]] == [[0, 3], [-1, 7]]
    # empty shapes on every path
    for mode in ("refuse", "auto", "sort"):
        codes, d, u = encoding.unique_codes(torch.zeros((0, 3), dtype=torch.int64), wide=mode, return_uniques=True)
        assert codes.shape == (0, 3) and d == [0, 0, 0] and [x.numel() for x in u] == [0, 0, 0]
    # a column that spans the whole int64 range is refused by default, not wrapped around
    with pytest.raises(NotImplementedError):
        encoding.unique_codes(torch.tensor([[I64_MIN], [I64_MAX]]))
    with pytest.raises(NotImplementedError):
        encoding.unique_codes(torch.tensor([[0.5]]), wide="sort")


def _wide_tensors():
    t1 = torch.tensor([[0, 5], [1 << 40, 5], [0, 6]])
    t2 = torch.tensor([[1 << 40, 9], [7, 5]])
    return [t1, t2]


def _numpy_fit(tensors):
    """utils_encoding.py:37-59 restated: np.unique per column over the concatenated rows, the inverse split per tensor"""
    cat = np.concatenate([t.numpy() for t in tensors], 0)
    d, corrs = [], {}
    for c in range(cat.shape[1]):
        u, inv = np.unique(cat[:, c], return_inverse=True)
        d.append(len(u))
        corrs[c] = inv
    out, ptr = [], 0
    for t in tensors:
        n = t.shape[0]
        out.append(np.stack([corrs[c][ptr:ptr + n] for c in range(cat.shape[1])], 1))
        ptr += n
    return d, corrs, out


def test_one_hot_unique_fits_wide_columns():
    tensors = _wide_tensors()
    enc = encoding.one_hot_unique(tensors)
    d, corrs, fitted = _numpy_fit(tensors)
    assert list(enc.d) == d
    assert sorted(enc.corrs) == sorted(corrs) and all(np.array_equal(enc.corrs[c], corrs[c]) for c in corrs)
    got = enc.fit(tensors)
    assert len(got) == len(fitted) and all(g.dtype == torch.int64 and np.array_equal(g.numpy(), f) for g, f in zip(got, fitted))
    assert [u.tolist() for u in enc.uniques] == [[0, 7, 1 << 40], [5, 6, 9]]


def test_encode_over_graphs_with_wide_identifiers():
    ids = [torch.tensor([[0, 2], [1 << 40, 3]]), torch.tensor([[1 << 40, 2]]), torch.tensor([[5, 2], [0, 1 << 62], [5, 3]])]
    graphs = []
    for t in ids:
        g = gdata.Data()
        g.identifiers = t.clone()
        graphs.append(g)
    graphs, enc_ids, d_id, enc_deg, d_deg = encoding.encode(graphs, "one_hot_unique", None, ids={})
    d, _, fitted = _numpy_fit(ids)
    assert list(d_id) == d and enc_deg is None and d_deg == []
    assert all(np.array_equal(g.identifiers.numpy(), f) for g, f in zip(graphs, fitted))


@pytest.mark.parametrize("path", ["table", "sort"])
def test_transform_on_fitted_permuted_and_repeated_rows(path):
    rng = np.random.default_rng(3)
    cat = rng.integers(-20, 40, size=(500, 3)).astype(np.int64)
    if path == "sort":
        cat[:, 1] = cat[:, 1] * (1 << 36)
        cat[0, 2], cat[1, 2] = I64_MIN, I64_MAX
    tensors = [torch.from_numpy(cat[:120]), torch.from_numpy(cat[120:120]), torch.from_numpy(cat[120:])]
    enc = encoding.one_hot_unique(tensors)
    for c in range(3):
        assert np.array_equal(enc.uniques[c].numpy(), np.unique(cat[:, c]))
    fit = enc.fit(tensors)
    got = enc.transform(tensors)
    assert len(got) == 3 and got[1].shape == (0, 3)             # (an empty tensor in the list)
    assert all(g.dtype == torch.int64 and not g.is_cuda and torch.equal(g, f) for g, f in zip(got, fit))
    perm = rng.permutation(500)
    rows = np.concatenate([perm, perm[:77], [perm[0]] * 5])
    got = enc.transform([torch.from_numpy(cat[rows])])[0]
    assert torch.equal(got, torch.cat(fit, 0)[rows])
    if path == "table":
        assert torch.equal(enc.transform([torch.from_numpy(cat[rows]).double()])[0], got)     # whole-number floats, as in fit
    with pytest.raises(NotImplementedError):
        enc.transform([torch.tensor([[0.5, 0.0, 0.0]])])


def test_transform_unseen_values():
    fitted = [torch.tensor([[10, -4], [20, 1 << 50], [40, -4]]), torch.tensor([[20, 7]])]
    enc = encoding.one_hot_unique(fitted)
    assert [u.tolist() for u in enc.uniques] == [[10, 20, 40], [-4, 7, 1 << 50]]
    new = [torch.tensor([[10, 7]]), torch.zeros((0, 2), dtype=torch.int64), torch.tensor([[40, -4], [20, 123456789012], [5, 7]])]
    with pytest.raises(ValueError) as e:
        enc.transform(new)
    msg = str(e.value)
    assert "123456789012" in msg and "column 1" in msg and "tensor 2" in msg and "row 1" in msg, msg
    with pytest.raises(ValueError):
        enc.transform(new, unknown="ignore")
    # clamp: below the smallest, between two fitted values, above the largest, and exact hits
    probe = np.array([[I64_MIN, I64_MIN], [9, -5], [10, -4], [11, -3], [39, 8], [40, 1 << 50], [41, (1 << 50) + 1], [I64_MAX, I64_MAX]], dtype=np.int64)
    got = enc.transform([torch.from_numpy(probe)], unknown="clamp")[0].numpy()
    for c in range(2):
        want = np.clip(np.searchsorted(enc.uniques[c].numpy(), probe[:, c], side="right") - 1, 0, None)
        assert np.array_equal(got[:, c], want), c
    # column-count mismatch: refused before anything is launched
    calls = _Recorder()
    with calls:
        with pytest.raises(ValueError):
            enc.transform([torch.tensor([[10, 7]]), torch.tensor([[10, 7, 1]])])
    assert calls.names == []


class _Recorder:
    """records the names of the library's entry points that are called while it is installed (gsn_amd._abi.lib() hands out _abi._lib)"""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call

    def __enter__(self):
        self.__dict__["_real"] = _abi.lib()
        _abi._lib = self
        return self

    def __exit__(self, *exc):
        _abi._lib = self._real
        return False


def test_lookup_codes_on_the_device():
    uniques = [torch.tensor([10, 20, 40]), torch.tensor([-4, 7, 1 << 50])]
    seen = torch.tensor([[40, 7], [10, -4], [20, 1 << 50]]).cuda()
    codes = encoding.lookup_codes(seen, uniques)
    assert codes.is_cuda and codes.tolist() == [[2, 1], [0, 0], [1, 2]]
    tables = encoding.lookup_tables(uniques, seen.device)
    codes, status = encoding.lookup_codes(seen, tables, check=False)
    assert codes.tolist() == [[2, 1], [0, 0], [1, 2]] and status.is_cuda and status.dtype == torch.int32 and int(status.item()) == 0
    unseen = torch.tensor([[40, 7], [10, 8], [30, -4]]).cuda()
    codes, status = encoding.lookup_codes(unseen, tables, check=False)
    assert int(status.item()) != 0 and codes.tolist() == [[2, 1], [0, -1], [-1, 0]]
    with pytest.raises(ValueError) as e:
        encoding.lookup_codes(unseen, tables)
    assert "value 8" in str(e.value) and "row 1" in str(e.value) and "column 1" in str(e.value)
    assert encoding.lookup_codes(unseen, tables, unknown="clamp").tolist() == [[2, 1], [0, 1], [1, 0]]
    with pytest.raises(ValueError):
        encoding.lookup_codes(seen[:, :1], tables)
    # R == 0: no entry point is called
    calls = _Recorder()
    with calls:
        codes, status = encoding.lookup_codes(torch.zeros((0, 2), dtype=torch.int64).cuda(), tables, check=False)
    assert calls.names == [] and codes.shape == (0, 2) and int(status.item()) == 0
    # a column with no fitted values: -1 and the status in strict mode, 0 in clamp mode
    empty = [torch.tensor([10, 20, 40]), torch.zeros(0, dtype=torch.int64)]
    codes, status = encoding.lookup_codes(seen, empty, check=False)
    assert int(status.item()) != 0 and codes.tolist() == [[2, -1], [0, -1], [1, -1]]
    assert encoding.lookup_codes(seen, empty, unknown="clamp").tolist() == [[2, 0], [0, 0], [1, 0]]
    none = [torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)]
    assert encoding.lookup_codes(seen, none, unknown="clamp").tolist() == [[0, 0]] * 3


def test_fit_on_a_dataset_without_rows():
    enc = encoding.one_hot_unique([torch.zeros((0, 3), dtype=torch.int64), torch.zeros((0, 3), dtype=torch.int64)])
    assert enc.d == [0, 0, 0] and len(enc.uniques) == 3 and all(u.numel() == 0 and u.dtype == torch.int64 for u in enc.uniques)
    assert [t.shape for t in enc.fit([torch.zeros((0, 3))])] == [(0, 3)]
    assert [t.shape for t in enc.transform([torch.zeros((0, 3), dtype=torch.int64)])] == [(0, 3)]
    with pytest.raises(ValueError):
        enc.transform([torch.tensor([[1, 2, 3]])])
    assert enc.transform([torch.tensor([[1, 2, 3]])], unknown="clamp")[0].tolist() == [[0, 0, 0]]
