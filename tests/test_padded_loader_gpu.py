"""GPU checks of the padded loader (gsn_amd.loader.PaddedDataLoader, gsn_loader_collate_padded_hip): every tensor of every batch byte for
byte against the referee tests/padded_ref.py with the static tensors poisoned with 0xFF in front of every launch (nothing of the previous
batch -- or of the poison -- may survive), the real prefix against the unpadded DataLoader, pointers that never move, the unfitting batch,
a segment longer than a wave pass, more than 256 graph slots, the refusals, and models in eval mode over a padded batch against the same
models over the unpadded batch.

The fixture datasets are ``make_dataset(11, 'A' / 'B')`` of tests/loader_ref.py -- 40 graphs of 1 - 70 vertices with a single-vertex graph,
edgeless graphs and 20-byte rows -- with graph 11's cut-short ``degrees`` restored to one row per vertex: a field that is neither per
vertex, per edge nor per graph has no padded layout and is refused (checked on the unmended dataset)."""
import types

import numpy as np
import pytest
import torch

from gsn_amd.data import Data
from loader_ref import collate_ref, make_dataset
from padded_models import DEV, molhiv_graphs, ogb_model, same_bytes, within_bar, zinc_graphs, zinc_model
from padded_ref import batches_of, padded_collate_ref, shape_ref

pytestmark = pytest.mark.gpu


def _mended(seed, variant):
    graphs = make_dataset(seed, variant)
    g = graphs[11]
    d = Data()
    for k, v in g:
        setattr(d, k, torch.arange(g.x.shape[0], dtype=torch.float32) % 5 if k == "degrees" else v)
    graphs[11] = d
    return graphs


@pytest.fixture(scope="module")
def datasets():
    return {v: _mended(11, v) for v in ("A", "B")}


def _sizes(graphs):
    return [int(g.x.shape[0]) for g in graphs], [int(g.edge_index.shape[1]) for g in graphs]


def _poison(loader):
    for t in loader.static_tensors():
        if t.numel():
            t.view(torch.uint8).fill_(0xFF)


def _assert_batch(got, want, where):
    """every attribute of the referee's batch, byte for byte"""
    for name, w in want:
        g = getattr(got, name)
        if isinstance(w, torch.Tensor):
            g = torch.from_numpy(g) if isinstance(g, np.ndarray) else g
            assert same_bytes(g, w), (where, name, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        else:
            assert g == w, (where, name, g, w)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("B", [1, 4, 7])
@pytest.mark.parametrize("variant", ["A", "B"])
def test_every_batch_against_the_referee(datasets, variant, B, shuffle):
    from gsn_amd.loader import Batch, DataLoader, DeviceDataset, PaddedBatch, PaddedDataLoader
    graphs = datasets[variant]
    ds = DeviceDataset(graphs)
    loader = PaddedDataLoader(ds, batch_size=B, shuffle=shuffle, generator=_gen(5) if shuffle else None)
    plain = DataLoader(ds, batch_size=B, shuffle=shuffle, generator=_gen(5) if shuffle else None)
    n, e = _sizes(graphs)
    sh = shape_ref(n, e, B, shuffle)
    assert (loader.node_capacity, loader.edge_capacity, loader.pad_slots, loader.graph_slots) == (sh["N_cap"], sh["E_cap"], sh["P"], sh["G_cap"])
    pointers, first = None, None
    for epoch in range(2):
        it, it_plain = iter(loader), iter(plain)
        order = loader.last_permutation.tolist()
        assert order == plain.last_permutation.tolist()
        assert sorted(order) == list(range(40)) and (shuffle or order == list(range(40)))
        for i, idx in enumerate(batches_of(40, B, False, order)):
            where = "%s B=%d shuffle=%s epoch %d batch %d" % (variant, B, shuffle, epoch, i)
            _poison(loader)
            batch = next(it)
            assert isinstance(batch, PaddedBatch) and batch.padded is True and (first is None or batch is first), where
            first = batch
            want = padded_collate_ref(graphs, idx, sh)
            assert want is not None, where
            _assert_batch(batch, want, where)
            assert int(batch.n_valid.item()) == len(idx) == batch.num_real_graphs
            part = batch.graph_partition
            assert part[0] is batch.ptr and same_bytes(part[1], want.edge_ptr) and part[2:] == (sh["n_chunk"], sh["e_chunk"], False), where
            # the real prefix is the unpadded batch of the same generator state
            real = next(it_plain)
            assert isinstance(real, Batch) and not getattr(real, "padded", False)
            b, N_r, E_r = len(idx), real.x.shape[0], real.edge_index.shape[1]
            kinds = {"node": N_r, "edge": E_r, "graph": b}
            for name in ds.field_names:
                t, r = getattr(batch, name), getattr(real, name)
                if name == "edge_index":
                    assert torch.equal(t[:, :E_r], r), (where, name)
                else:
                    rows = r.shape[0]
                    assert rows in kinds.values() and torch.equal(t[:rows], r), (where, name)
            assert torch.equal(batch.batch[:N_r], real.batch) and torch.equal(batch.ptr[:b + 1], real.ptr)
            assert np.array_equal(batch.node_ptr[:b + 1], real.node_ptr) and np.array_equal(batch.edge_ptr[:b + 1], real.edge_ptr)
            now = [t.data_ptr() for t in loader.static_tensors()] + [getattr(batch, k).data_ptr() for k in ds.field_names + ["batch", "ptr", "n_valid"]]
            assert pointers is None or now == pointers, where
            pointers = now
        with pytest.raises(StopIteration):
            next(it)


def test_a_batch_that_does_not_fit_is_an_ordinary_batch(datasets):
    from gsn_amd.loader import Batch, PaddedBatch, PaddedDataLoader
    graphs = datasets["A"]
    n, e = _sizes(graphs)
    B = 7
    totals = [(sum(n[i] for i in idx), sum(e[i] for i in idx)) for idx in batches_of(40, B)]
    e_cap = sorted(t[1] for t in totals)[-2]                      # the batch with the most edge columns misses it
    loader = PaddedDataLoader(graphs, batch_size=B, edge_capacity=e_cap, fill={"y": -3.5, "identifiers": 8})
    sh = shape_ref(n, e, B, edge_capacity=e_cap)
    assert loader.edge_capacity == e_cap and loader.node_capacity == sh["N_cap"]
    seen = []
    for i, (idx, batch) in enumerate(zip(batches_of(40, B), loader)):
        want = padded_collate_ref(graphs, idx, sh, fill={"y": -3.5, "identifiers": 8})
        seen.append(want is not None)
        if want is None:
            assert type(batch) is Batch and not getattr(batch, "padded", False)
            ref = collate_ref(graphs, idx)
            for name, w in ref:
                g = getattr(batch, name)
                if isinstance(w, torch.Tensor):
                    g = torch.from_numpy(g) if isinstance(g, np.ndarray) else g
                    assert same_bytes(g, w), (i, name)
                else:
                    assert g == w, (i, name)
        else:
            assert isinstance(batch, PaddedBatch)
            _assert_batch(batch, want, "batch %d" % i)
    assert seen.count(False) == 1 and seen.count(True) == len(totals) - 1


def test_long_segments_and_more_than_256_slots():
    from gsn_amd.loader import PaddedDataLoader
    rng = np.random.default_rng(3)
    graphs = make_dataset(4, "A")[:5]
    n, E = 300, 700
    big = Data()                                                   # (attributes in the order of the fixture's graphs)
    big.edge_index = torch.from_numpy(rng.integers(0, n, (2, E)).astype(np.int64))
    big.x = torch.from_numpy(rng.integers(0, 28, (n, 1)).astype(np.int64))
    big.graph_size = n
    big.degrees = torch.from_numpy(rng.integers(0, 5, n).astype(np.float32))
    big.edge_features = torch.from_numpy(rng.integers(0, 4, E).astype(np.int64))
    big.y = torch.from_numpy(rng.standard_normal(1).astype(np.float32))
    big.identifiers = torch.from_numpy(rng.integers(0, 9, (E, 5)).astype(np.int64))
    assert [k for k, _ in big] == [k for k, _ in graphs[0]]
    graphs = graphs[:2] + [big] + graphs[2:]
    ns, es = _sizes(graphs)
    for B in (4, 6):                                               # (the small batches get pad graphs of up to 300 vertices / 700 loops)
        sh = shape_ref(ns, es, B)
        loader = PaddedDataLoader(graphs, batch_size=B)
        it = iter(loader)
        for idx in batches_of(len(graphs), B):
            _poison(loader)
            _assert_batch(next(it), padded_collate_ref(graphs, idx, sh), "long B=%d %s" % (B, idx))
    # 300 single-vertex graphs in one batch: G_cap > 256 slots, n_chunk = 2
    many = []
    for g in range(300):
        d = Data()
        m = int(rng.integers(0, 3))
        d.edge_index = torch.zeros((2, m), dtype=torch.int64)
        d.x = torch.from_numpy(rng.integers(0, 28, (1, 1)).astype(np.int64))
        d.degrees = torch.from_numpy(rng.integers(0, 5, 1).astype(np.float32))
        d.edge_features = torch.from_numpy(rng.integers(0, 4, m).astype(np.int64))
        d.y = torch.from_numpy(rng.standard_normal(1).astype(np.float32))
        d.graph_size = 1
        many.append(d)
    ns, es = _sizes(many)
    for B, shuffle in ((300, False), (300, True), (299, False)):
        sh = shape_ref(ns, es, B, shuffle)
        assert sh["G_cap"] > 256 and sh["n_chunk"] == 2
        loader = PaddedDataLoader(many, batch_size=B, shuffle=shuffle, generator=_gen(1) if shuffle else None)
        it = iter(loader)
        for idx in batches_of(300, B, False, loader.last_permutation.tolist()):
            _poison(loader)
            batch = next(it)
            want = padded_collate_ref(many, idx, sh)
            _assert_batch(batch, want, "many B=%d %d graphs" % (B, len(idx)))
            # y shares x's row pointer here (one row per graph either way): it is per graph, degrees per vertex
            assert batch.y.shape[0] == sh["G_cap"] and batch.degrees.shape[0] == sh["N_cap"]


def test_refusals_and_iterators(datasets):
    from gsn_amd.loader import PaddedDataLoader
    with pytest.raises(ValueError, match="degrees"):
        PaddedDataLoader(make_dataset(11, "A"), batch_size=4)           # graph 11's degrees are cut short: no padded layout
    with pytest.raises(ValueError, match="nope"):
        PaddedDataLoader(datasets["A"], batch_size=4, fill={"nope": 1})
    loader = PaddedDataLoader(datasets["B"], batch_size=16)
    it = iter(loader)
    next(it)
    with pytest.raises(RuntimeError, match="iterator"):
        iter(loader)
    with pytest.raises(RuntimeError, match="iterator"):
        list(zip(loader, loader))
    list(it)                                                            # finished: the next epoch may start
    assert len(list(loader)) == 3
    it = iter(loader)
    next(it)
    del it                                                              # dropped unfinished: gone, not alive
    assert len(list(loader)) == 3


def _unpadded(graphs, idx):
    ref = collate_ref(graphs, idx)
    return types.SimpleNamespace(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ref})


@pytest.mark.parametrize("which", ["zinc", "ogb"])
def test_models_in_eval_mode_over_a_padded_batch(which):
    """rows [:b] of model(padded batch) against model(unpadded batch) within the element-wise bar; all pad rows finite; training mode raises"""
    from gsn_amd.loader import PaddedDataLoader
    graphs, model = (zinc_graphs(), zinc_model()) if which == "zinc" else (molhiv_graphs(20, False), ogb_model())
    loader = PaddedDataLoader(graphs, batch_size=12)
    n_batches = 0
    with torch.no_grad():
        for idx, batch in zip(batches_of(len(graphs), 12), loader):
            b = len(idx)
            y = model(batch)
            assert y.shape == (loader.graph_slots, 1) and batch.num_graphs == loader.graph_slots
            y_ref = model(_unpadded(graphs, idx))
            assert y_ref.shape == (b, 1)
            assert within_bar(y[:b], y_ref), (which, idx[0], float((y[:b] - y_ref).abs().max()))
            assert bool(torch.isfinite(y).all()), (which, idx[0])
            n_batches += 1
    assert n_batches == len(loader) == (3 if which == "zinc" else 2) and b == 8
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model(next(iter(loader)))
    model.eval()
