"""evaluation.GraphedEpoch on the GPU: ``test`` / ``test_ogb`` over a PaddedDataLoader (one collate launch and one graph replay per batch)
against the same over the unpadded DataLoader (the eager loop), on the ZINC-shaped GNNSubstructures and on a molhiv-shaped GNN_OGB with
virtual node and 20 % NaN labels.  The replayed graph must compute with the parameters AS THEY ARE at the replay -- after an optimizer step,
after load_state_dict, after somebody else's invalidate_caches and eager forwards -- which is what a capture that found warm derived-weight
caches would get wrong; with one capture per (model, loader) over all of it."""
import types

import numpy as np
import pytest
import torch

from eval_ref import rank_ref
from gsn_amd import evaluation as ev, layers
from loader_ref import collate_ref
from padded_models import DEV, molhiv_graphs, ogb_model, same_bytes, within_bar, zinc_code_model, zinc_graphs, zinc_model
from padded_ref import shape_ref

pytestmark = pytest.mark.gpu
BAR = 2e-5          # a single number: 1e-5 |b| + 1e-5 max|b| (tests/test_loader_gpu.py)


def _close(got, want):
    return abs(float(got) - float(want)) <= BAR * abs(float(want))


def _train_step(model, graphs, lr=2e-2):
    """one Adam step in training mode over an UNPADDED batch: parameters and BatchNorm running statistics move"""
    ref = collate_ref(graphs, list(range(10)))
    data = types.SimpleNamespace(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ref})
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    model.train()
    opt.zero_grad()
    (model(data) - 1.0).square().mean().backward()
    opt.step()
    model.eval()


def test_zinc_epochs_follow_the_live_parameters():
    from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader
    graphs = zinc_graphs()
    ds = DeviceDataset(graphs)
    model = zinc_model()
    plain, padded = DataLoader(ds, batch_size=12), PaddedDataLoader(ds, batch_size=12)
    assert len(padded) == 3

    def both(n_iters=None):
        want = ev.test(plain, model, "L1Loss", DEV, prediction_fn="L1Loss", n_iters=n_iters)
        got = ev.test(padded, model, "L1Loss", DEV, prediction_fn="L1Loss", n_iters=n_iters)
        assert _close(got[0], want[0]) and _close(got[1], want[1]), (got, want)
        return got

    first = both()
    (epoch,) = padded.graphed_epochs.values()
    assert isinstance(epoch, ev.GraphedEpoch) and epoch.captures == 1 and epoch.replays == 3 and epoch.eager_batches == 0
    again = both()
    assert _close(again[0], first[0]) and _close(again[1], first[1])
    # the stale-derived-weights trap: an optimizer step between epochs
    _train_step(model, graphs)
    second = both()
    assert abs(second[0] - first[0]) > 1e-3 * abs(first[0]), (first, second)
    # other weights through load_state_dict
    other = zinc_model(seed=3)
    model.load_state_dict(other.state_dict())
    third = both()
    assert abs(third[0] - second[0]) > 1e-3 * abs(second[0]), (second, third)
    # somebody else's invalidate_caches and an eager forward on other data in between, then a write the version counters do not see
    layers.invalidate_caches(model)
    with torch.no_grad():
        model(next(iter(DataLoader(ds, batch_size=5))))
        for p in model.parameters():
            p.data.mul_(1.25)
    layers.invalidate_caches(model)                               # (what a write through .data asks of the EAGER path)
    fourth = both()
    assert abs(fourth[0] - third[0]) > 1e-3 * abs(third[0]), (third, fourth)
    # n_iters beyond one pass wraps round as the eager loop does
    wrapped = both(n_iters=5)
    assert wrapped[0] > fourth[0]
    assert ev.test(padded, model, "L1Loss", DEV, prediction_fn="L1Loss", n_iters=1)[0] < fourth[0]
    assert list(padded.graphed_epochs.values()) == [epoch] and epoch.captures == 1
    # a GraphedEpoch of one's own; training mode is refused
    own = ev.GraphedEpoch(model, PaddedDataLoader(ds, batch_size=12), "L1Loss", "L1Loss")
    mine = own.run()
    assert _close(mine[0], fourth[0]) and _close(mine[1], fourth[1]) and own.captures == 1
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        own.run()
    model.eval()
    with pytest.raises(TypeError):
        ev.GraphedEpoch(model, plain, "L1Loss")


def test_a_batch_that_does_not_fit_runs_eagerly_into_the_same_sums():
    from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader
    graphs = zinc_graphs()
    ds = DeviceDataset(graphs)
    model = zinc_model()
    n = [int(g.x.shape[0]) for g in graphs]
    e = [int(g.edge_index.shape[1]) for g in graphs]
    per_batch = sorted(sum(e[i:i + 12]) for i in (0, 12))        # the two full batches; the larger one misses the capacity
    assert per_batch[0] < per_batch[1]
    padded = PaddedDataLoader(ds, batch_size=12, edge_capacity=per_batch[0])
    sh = shape_ref(n, e, 12, edge_capacity=per_batch[0])
    assert padded.node_capacity == sh["N_cap"]
    want = ev.test(DataLoader(ds, batch_size=12), model, "L1Loss", DEV, prediction_fn="L1Loss")
    for _ in range(2):
        got = ev.test(padded, model, "L1Loss", DEV, prediction_fn="L1Loss")
        assert _close(got[0], want[0]) and _close(got[1], want[1]), (got, want)
    (epoch,) = padded.graphed_epochs.values()
    assert epoch.captures == 1 and epoch.replays == 4 and epoch.eager_batches == 2


def test_a_model_whose_first_layer_runs_on_integer_codes():
    """layer 0 on code keys: its code-gather stages read an out-of-range flag back in an eager forward, which a capture cannot"""
    from gsn_amd import flags
    from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader
    ds = DeviceDataset(zinc_graphs())
    model = zinc_code_model()
    padded = PaddedDataLoader(ds, batch_size=12)
    assert flags.CODE_STATUS_CHECK
    for _ in range(2):
        want = ev.test(DataLoader(ds, batch_size=12), model, "L1Loss", DEV, prediction_fn="L1Loss")
        got = ev.test(padded, model, "L1Loss", DEV, prediction_fn="L1Loss")
        assert _close(got[0], want[0]) and _close(got[1], want[1]), (got, want)
        _train_step(model, zinc_graphs(), lr=1e-3)
    assert flags.CODE_STATUS_CHECK                              # (off for the capture only)
    (epoch,) = padded.graphed_epochs.values()
    assert epoch.captures == 1 and epoch.replays == 6


class _Recording(ev.Evaluator):
    def eval(self, input_dict):
        self.seen = {k: v.clone() for k, v in input_dict.items()}
        return super().eval(input_dict)


def test_molhiv_epochs_with_nan_labels_and_the_skip_rule():
    from gsn_amd.loader import DataLoader, DeviceDataset, PaddedDataLoader
    graphs = molhiv_graphs()                                      # 25 graphs: batches of 12, 12 and one single-vertex graph (skipped)
    ds = DeviceDataset(graphs)
    model = ogb_model()
    plain, padded = DataLoader(ds, batch_size=12), PaddedDataLoader(ds, batch_size=12)
    loss_fn = ev.MaskedLoss("BCEWithLogitsLoss")
    ev_plain, ev_padded = _Recording("ogbg-molhiv"), _Recording("ogbg-molhiv")

    def both(n_iters=None, rows=24):
        want = ev.test_ogb(plain, model, loss_fn, DEV, ev_plain, n_iters=n_iters)
        got = ev.test_ogb(padded, model, loss_fn, DEV, ev_padded, n_iters=n_iters)
        a, b = ev_padded.seen, ev_plain.seen
        assert a["y_true"].shape == (rows, 1) and same_bytes(a["y_true"], b["y_true"])
        assert within_bar(a["y_pred"], b["y_pred"]), float((a["y_pred"] - b["y_pred"]).abs().max())
        assert _close(got[0], want[0]), (got, want)
        r = rank_ref(a["y_pred"].cpu().numpy()[:, 0], a["y_true"].cpu().numpy()[:, 0])
        assert got[1] == r["auc"], (got, r)                      # the metric of the graphed path's own gathered rows, exactly
        return got

    first = both()
    (epoch,) = padded.graphed_epochs.values()
    assert epoch.captures == 1 and epoch.replays == 2 and epoch.eager_batches == 0
    _train_step(model, graphs)
    second = both()
    assert abs(second[0] - first[0]) > 1e-3 * abs(first[0]), (first, second)
    layers.invalidate_caches(model)
    with torch.no_grad():
        model(next(iter(DataLoader(ds, batch_size=7))))
    model.load_state_dict(ogb_model(seed=4).state_dict())
    third = both()
    assert abs(third[0] - second[0]) > 1e-3 * abs(second[0]), (second, third)
    both(n_iters=5, rows=48)                                      # 12, 12, skipped, 12, 12: the rows of the first pass are moved out
    assert list(padded.graphed_epochs.values()) == [epoch] and epoch.captures == 1
