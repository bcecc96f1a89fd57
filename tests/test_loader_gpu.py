"""The device-resident loader on the GPU (gsn_amd/loader.py, csrc/loader.hip: one launch per collated batch) against the CPU referee
tests/loader_ref.py.  Every comparison of a batch is exact (``torch.equal``, dtype and shape included); the two integration tests compare
model outputs within the project's element-wise bar |a - b| <= 1e-5 |b| + 1e-5 max|b row| (README, round 3)."""
import types

import networkx as nx
import numpy as np
import pytest
import torch

from gsn_amd.data import Data
from loader_ref import assert_batch_equal, collate_ref, make_dataset

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures():
    from gsn_amd.loader import DeviceDataset
    out = {}
    for v in ("A", "B"):
        graphs = make_dataset(11, v)
        out[v] = (graphs, DeviceDataset(graphs, device=DEV))
    return out


def check_batch(batch, graphs, idx, where=""):
    """``batch`` (a loader's) is the referee's collation of ``graphs[idx]`` in every field, pointer and size."""
    ref = collate_ref(graphs, idx)
    assert_batch_equal(batch, ref, where)                    # fields, batch, ptr, edge_ptr, num_graphs
    assert isinstance(batch.node_ptr, np.ndarray) and batch.node_ptr.dtype == np.int64 and batch.node_ptr.tolist() == ref.ptr.tolist(), where
    assert isinstance(batch.edge_ptr, np.ndarray) and batch.edge_ptr.dtype == np.int64 and batch.edge_ptr.tolist() == ref.edge_ptr.tolist(), where
    assert batch.ptr.is_cuda and batch.batch.is_cuda
    part = batch.graph_partition
    assert len(part) == 5 and part[0] is batch.ptr and part[4] is False, where
    assert part[1].is_cuda and part[1].dtype == torch.int64 and part[1].cpu().tolist() == ref.edge_ptr.tolist(), where
    assert part[2] == int(ref.ptr.diff().max()) and part[3] == int(ref.edge_ptr.diff().max()), where
    for name, v in batch:
        if isinstance(v, torch.Tensor):
            assert v.device == DEV and v.is_contiguous(), (where, name)
    assert batch.to(DEV) is batch and batch.to("cuda") is batch
    return ref


def check_epoch(loader, graphs, where=""):
    it = iter(loader)
    perm = loader.last_permutation
    assert perm.dtype == torch.int64 and not perm.is_cuda and sorted(perm.tolist()) == list(range(len(graphs)))
    bs = loader.batch_size
    n = 0
    for i, batch in enumerate(it):
        idx = perm[i * bs:(i + 1) * bs].tolist()
        check_batch(batch, graphs, idx, "%s batch %d" % (where, i))
        n += 1
    assert n == len(loader), where
    return perm


@pytest.mark.parametrize("batch_size", [1, 7, 40, 64])
@pytest.mark.parametrize("variant", ["A", "B"])
def test_every_batch_equals_the_referee(fixtures, variant, batch_size):
    from gsn_amd.loader import DataLoader
    graphs, ds = fixtures[variant]
    assert len(ds) == 40
    for shuffle in (False, True):
        for drop_last in (False, True):
            gen = torch.Generator()
            gen.manual_seed(batch_size)
            loader = DataLoader(ds, batch_size=batch_size, shuffle=shuffle, drop_last=drop_last, generator=gen)
            assert loader.dataset is ds and loader.batch_size == batch_size
            assert len(loader) == (40 // batch_size if drop_last else -(-40 // batch_size))
            where = "%s bs %d shuffle %d drop_last %d" % (variant, batch_size, shuffle, drop_last)
            p0 = check_epoch(loader, graphs, where)
            p1 = check_epoch(loader, graphs, where + " (second epoch)")
            if shuffle:
                assert p0.tolist() != p1.tolist()
            else:
                assert p0.tolist() == list(range(40)) == p1.tolist()


def test_a_list_of_graphs_is_wrapped(fixtures):
    from gsn_amd.loader import DataLoader, DeviceDataset
    graphs = fixtures["A"][0][:9]
    loader = DataLoader(graphs, batch_size=4)
    assert isinstance(loader.dataset, DeviceDataset) and len(loader.dataset) == 9 and len(loader) == 3
    check_epoch(loader, graphs, "wrapped list")


@pytest.mark.parametrize("batch_size", [7, 3])
def test_long_segments(batch_size):
    """a 3 000-vertex / 10 000-column graph among tiny ones: segments many times longer than one pass of a wave"""
    from gsn_amd.loader import DataLoader
    graphs = make_dataset(5, "long")
    assert max(g.x.shape[0] for g in graphs) == 3000 and max(g.edge_index.shape[1] for g in graphs) == 10000
    gen = torch.Generator()
    gen.manual_seed(1)
    for shuffle in (False, True):
        check_epoch(DataLoader(graphs, batch_size=batch_size, shuffle=shuffle, generator=gen), graphs, "long bs %d" % batch_size)


def test_many_slots():
    """5 000 graphs at batch_size 4 096: more (field, slot) pairs than the grid has waves, so the grid-stride loop runs more than once"""
    from gsn_amd.loader import DataLoader
    graphs = make_dataset(6, "many")
    gen = torch.Generator()
    gen.manual_seed(2)
    loader = DataLoader(graphs, batch_size=4096, shuffle=True, generator=gen)
    assert len(loader) == 2 and 7 * 4096 > 2048 * 4
    check_epoch(loader, graphs, "many")


def _clone_batch(batch):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in batch if k != "graph_partition"}


def test_batches_are_not_aliased(fixtures):
    from gsn_amd.loader import DataLoader
    graphs, ds = fixtures["A"]
    gen = torch.Generator()
    gen.manual_seed(3)
    loader = DataLoader(ds, batch_size=7, shuffle=True, generator=gen)
    it = iter(loader)
    first = next(it)
    idx = loader.last_permutation[:7].tolist()
    saved = _clone_batch(first)
    torch.cuda.synchronize()
    rest = list(it)
    second = list(loader)
    torch.cuda.synchronize()
    assert len(rest) == 5 and len(second) == 6
    for k, v in saved.items():
        now = getattr(first, k)
        if isinstance(v, torch.Tensor):
            assert torch.equal(now, v), k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(now, v), k
        else:
            assert now == v, k
    check_batch(first, graphs, idx, "batch 0 after two epochs")
    ptrs = {t.data_ptr() for b in [first] + rest + second for _, t in b if isinstance(t, torch.Tensor) and t.numel()}
    assert len(ptrs) == sum(1 for b in [first] + rest + second for _, t in b if isinstance(t, torch.Tensor) and t.numel())


def test_two_live_iterators(fixtures):
    from gsn_amd.loader import DataLoader
    graphs, ds = fixtures["B"]
    gen = torch.Generator()
    gen.manual_seed(4)
    loader = DataLoader(ds, batch_size=7, shuffle=True, generator=gen)
    it_a = iter(loader)
    perm_a = loader.last_permutation.clone()
    it_b = iter(loader)
    perm_b = loader.last_permutation.clone()
    assert perm_a.tolist() != perm_b.tolist()
    pairs = list(zip(it_a, it_b))
    assert len(pairs) == 6
    for i, (a, b) in enumerate(pairs):
        check_batch(a, graphs, perm_a[i * 7:(i + 1) * 7].tolist(), "iterator a, batch %d" % i)
        check_batch(b, graphs, perm_b[i * 7:(i + 1) * 7].tolist(), "iterator b, batch %d" % i)
    seq = DataLoader(ds, batch_size=16)
    for i, (a, b) in enumerate(zip(seq, seq)):
        check_batch(a, graphs, list(range(16 * i, min(16 * i + 16, 40))), "sequential a")
        check_batch(b, graphs, list(range(16 * i, min(16 * i + 16, 40))), "sequential b")


@pytest.mark.parametrize("variant", ["A", "B"])
def test_indexing_and_subsets(fixtures, variant):
    from gsn_amd.loader import DataLoader, DeviceDataset
    graphs, ds = fixtures[variant]
    for i, g in enumerate(graphs):
        d = ds[i]
        assert isinstance(d, Data) and d.keys == g.keys
        for k, v in g:
            got = getattr(d, k)
            if isinstance(v, torch.Tensor):
                assert got.device == DEV and got.dtype == v.dtype and got.shape == v.shape and torch.equal(got.cpu(), v), (i, k)
            else:
                assert type(got) is type(v) and got == v, (i, k)
    idx = [5, 3, 19, 38, 0, 11, 7, 22, 5]
    sub = ds.subset(idx)
    assert isinstance(sub, DeviceDataset) and len(sub) == len(idx)
    for name in ds.field_names:
        assert sub.field_storage(name).data_ptr() == ds.field_storage(name).data_ptr(), name      # no second copy
        assert sub.host_sizes(name).dtype == np.int64
    assert sub.host_sizes("x").tolist() == [graphs[i].x.shape[0] for i in idx]
    assert torch.equal(sub[2].x.cpu(), graphs[19].x)
    chosen = [graphs[i] for i in idx]
    gen = torch.Generator()
    gen.manual_seed(6)
    for shuffle in (False, True):
        check_epoch(DataLoader(sub, batch_size=4, shuffle=shuffle, generator=gen), chosen, "subset")
    check_epoch(DataLoader(sub.subset([8, 0, 1]), batch_size=2), [chosen[8], chosen[0], chosen[1]], "subset of a subset")


def _within_bar(a, b):
    a, b = a.detach().double().cpu().reshape(b.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    bar = 1e-5 * b.abs() + 1e-5 * b.abs().max(dim=1, keepdim=True).values
    return bool(((a - b).abs() <= bar).all())


@pytest.fixture(scope="module")
def zinc_graphs():
    """32 ZINC-shaped prepared graphs: atom / bond codes, cycle identifiers (GSN-e, k <= 6) from the counting kernel, a regression target"""
    from gsn_amd import synth
    from gsn_amd.counting import counts2ids_batch
    b = synth.zinc_shape_batch(32, seed=77)
    pats = [list(nx.cycle_graph(k).edges) for k in range(3, 7)]
    ids = counts2ids_batch(b, pats, "edge", False, device=DEV).cpu().clamp(max=2)
    rng = np.random.default_rng(7)
    graphs = []
    for g in range(b.num_graphs):
        n0, n1, e0, e1 = int(b.node_ptr[g]), int(b.node_ptr[g + 1]), int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        d = Data()
        d.edge_index = torch.from_numpy(b.edge_index[:, e0:e1] - n0)
        d.x = torch.from_numpy(b.atom_type[n0:n1]).unsqueeze(1)
        d.graph_size = n1 - n0
        d.degrees = torch.zeros(n1 - n0)
        d.edge_features = torch.from_numpy(b.bond_type[e0:e1]).unsqueeze(1)
        d.y = torch.from_numpy(rng.standard_normal(1).astype(np.float32))
        d.identifiers = ids[e0:e1].clone()
        graphs.append(d)
    return graphs


def test_model_and_evaluation_over_a_loader(zinc_graphs):
    """The ZINC configuration of tests/test_model_gpu.py in eval mode: a loader batch (with its graph_partition) against the referee batch
    moved to the device (without one), and evaluation.test over the loader against the same sums from the referee batches."""
    from gsn_amd import evaluation, models
    from gsn_amd.loader import DataLoader
    from test_model_gpu import _kwargs
    kw = _kwargs("GSN_edge_sparse", 3, 32, "general", "local", True, False, "mean", "relu", False, "one_hot_encoder", "one_hot_encoder",
                 "one_hot_encoder", 16)
    torch.manual_seed(0)
    model = models.GNNSubstructures(1, 1, None, [3, 3, 3, 3], 1, [28], [4], **kw).to(DEV).eval()
    loader = DataLoader(zinc_graphs, batch_size=12)
    assert len(loader) == 3
    refs, outs_ref, n = [], [], len(zinc_graphs)
    with torch.no_grad():
        for i, batch in enumerate(loader):
            idx = list(range(12 * i, min(12 * i + 12, n)))
            ref = check_batch(batch, zinc_graphs, idx, "zinc batch %d" % i)
            on_dev = types.SimpleNamespace(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ref})
            assert not hasattr(on_dev, "graph_partition")
            y_ref = model(on_dev)
            y = model(batch)
            assert y.shape == (len(idx), 1) and y_ref.shape == y.shape
            assert _within_bar(y, y_ref), (i, float((y - y_ref).abs().max()))
            refs.append(ref)
            outs_ref.append(y_ref.double().cpu())
    loss_sum = sum(float((o.reshape(-1) - r.y.double()).abs().mean()) * r.num_graphs for o, r in zip(outs_ref, refs))
    metric_sum = sum(float((o.reshape(-1) - r.y.double()).abs().sum()) for o, r in zip(outs_ref, refs))
    loss, metric = evaluation.test(loader, model, "L1Loss", DEV, prediction_fn="L1Loss")
    for got, want in ((float(loss), loss_sum / n), (float(metric), metric_sum / n)):
        assert abs(got - want) <= 2e-5 * abs(want), (got, want)      # the bar for a single number: 1e-5 |b| + 1e-5 max|b|


def test_dgn_graph_from_a_loader_batch(zinc_graphs):
    from gsn_amd import dgn
    from gsn_amd.loader import DataLoader
    loader = DataLoader(zinc_graphs, batch_size=20)
    batch = next(iter(loader))
    ref = collate_ref(zinc_graphs, list(range(20)))
    host = types.SimpleNamespace(edge_index=ref.edge_index, node_ptr=ref.ptr.numpy(), edge_ptr=ref.edge_ptr.numpy())
    g = dgn.DGNGraph.from_batch(batch, edge_field=batch.identifiers, device=DEV)
    g_ref = dgn.DGNGraph.from_batch(host, edge_field=ref.identifiers, device=DEV)
    assert g.num_graphs == g_ref.num_graphs == 20 and g.num_nodes == g_ref.num_nodes
    assert torch.equal(g.batch, g_ref.batch) and torch.equal(g.batch, batch.batch)
    assert torch.equal(g.snorm_n, g_ref.snorm_n) and torch.equal(g.edge_index, g_ref.edge_index)
    assert torch.equal(g.edata["eig"], g_ref.edata["eig"])
    assert np.array_equal(g.node_ptr, g_ref.node_ptr) and np.array_equal(g.edge_ptr, g_ref.edge_ptr)
