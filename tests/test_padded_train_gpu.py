"""Training on padded batches: under ``loader.masked_training(batch)`` a training step on a padded batch is, up to summation
order, the step on the unpadded batch of the same graphs -- loss, every parameter gradient, BatchNorm running statistics and counters -- and
``graphs.PaddedTrainStep`` replays that step as one captured graph per batch.

The measure is the one of tests/test_graphed_train_gpu.py (_rel): the adjoints accumulate with floating-point atomics, so two eager runs
from the same state already differ in the last bits; ``noise`` is that difference, measured here, and the bar is max(16 noise, 2e-5)."""
import types

import pytest
import torch

from loader_ref import collate_ref
from padded_models import DEV, molhiv_graphs, ogb_model, zinc_graphs, zinc_model
from padded_ref import batches_of
from test_graphed_train_gpu import _rel

pytestmark = pytest.mark.gpu
B = 12


def _setup(which):
    if which == "zinc":
        return zinc_graphs(), zinc_model(), "L1Loss"
    return molhiv_graphs(20, False), ogb_model(), "BCEWithLogitsLoss"


def _unpadded(graphs, idx):
    ref = collate_ref(graphs, idx)
    return types.SimpleNamespace(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ref})


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _one_step(model, state0, forward_loss, dropout_seed=None):
    """loss, parameter gradients and BatchNorm buffers after ONE training forward + backward from ``state0`` (``dropout_seed``: native
    dropout's device state is put to (seed, 0 calls) first)"""
    model.load_state_dict(state0)
    if dropout_seed is not None:
        from gsn_amd.dropout import default_state
        default_state(torch.device(DEV, 0)).manual_seed(dropout_seed)
    model.train()
    model.zero_grad(set_to_none=True)
    loss = forward_loss()
    loss.backward()
    out = {"loss": loss.detach().clone().reshape(1)}
    for k, p in model.named_parameters():
        out["grad." + k] = torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()
    for k, b in model.named_buffers():
        out["buffer." + k] = b.detach().clone()
    torch.cuda.synchronize()
    model.eval()
    return out


def _grads_only(s):
    return {k: v for k, v in s.items() if k.startswith("grad.")}


def _check_step(which, loader_kw, native_dropout=None):
    from gsn_amd import evaluation as ev
    from gsn_amd.loader import PaddedDataLoader, masked_training
    graphs, model, kind = _setup(which)
    seed = None
    if native_dropout is not None:
        model.dropout_impl, model.dropout_features, seed = "native", [native_dropout] * len(model.dropout_features), 4321
    state0 = _snapshot(model)
    loader = PaddedDataLoader(graphs, batch_size=B, **loader_kw)
    seen = []
    for idx, batch in zip(batches_of(len(graphs), B), loader):
        assert getattr(batch, "padded", False), "the batch did not fit the capacities of this test"
        if len(idx) == B and B in seen:
            continue                              # (the full batch and the short last one: one of each)
        seen.append(len(idx))
        data = _unpadded(graphs, idx)

        def eager():
            return ev.masked_loss(kind, model(data), data.y)

        def padded():
            with masked_training(batch):
                pred = model(batch)
            return ev.masked_loss(kind, pred, batch.y, n_valid=batch.n_valid)

        plain = types.SimpleNamespace(**{k: v for k, v in batch})      # the same padded tensors, handed over as an ordinary batch: statistics over ALL rows

        def leaky():
            return ev.masked_loss(kind, model(plain), batch.y, n_valid=batch.n_valid)

        a, a2 = _one_step(model, state0, eager, seed), _one_step(model, state0, eager, seed)
        b = _one_step(model, state0, padded, seed)
        noise = _rel(a, a2)
        diff = _rel(a, b)
        bar = max(16.0 * noise, 2e-5)
        print("padded-train %s b = %d: diff %.3g at %s, eager run-to-run %.3g, bar %.3g" % (which, len(idx), diff, _rel.where, noise, bar))
        assert diff <= bar, "padded step differs from the unpadded one: %.3g at %s (bar %.3g)" % (diff, _rel.where, bar)
        nbt = [k for k in b if k.endswith("num_batches_tracked")]
        assert nbt and all(torch.equal(a[k], b[k]) for k in nbt)
        # the discriminating figure: without the bounds the pad rows enter the statistics and the gradients are somebody else's
        c = _one_step(model, state0, leaky, seed)
        leak = _rel(_grads_only(a), _grads_only(c))
        print("padded-train %s b = %d: statistics over all rows move the gradients by %.3g" % (which, len(idx), leak))
        assert leak > 100.0 * bar, "the comparison does not tell masked from unmasked statistics: %.3g vs bar %.3g" % (leak, bar)
    assert sorted(seen) == [8, B]
    model.load_state_dict(state0)


@pytest.mark.parametrize("which", ["zinc", "ogb"])
def test_one_training_step_padded_equals_unpadded(which):
    _check_step(which, {})


def test_equal_node_and_edge_capacities():
    """the row class of a stage is named by its call site, never read off a row count: with N_cap == E_cap nothing can be told from the shape"""
    from gsn_amd.loader import PaddedDataLoader
    graphs = zinc_graphs()
    auto = PaddedDataLoader(graphs, batch_size=B)
    cap = max(auto.node_capacity, auto.edge_capacity) + 64
    _check_step("zinc", {"node_capacity": cap, "edge_capacity": cap})


def test_native_dropout_draws_the_unpadded_masks_on_the_real_rows():
    """csrc/dropout_core.h indexes Philox by the linear element of the [rows, C] tensor, counted from its start: the real rows of a padded
    tensor are a prefix, so at equal DropoutState they draw the masks of the unpadded tensor (p = 0.5, every layer and the virtual node)"""
    _check_step("ogb", {}, native_dropout=0.5)


def _biases_in_front_of_batchnorm(model):
    """state-dict names of the Linear biases whose output goes straight into a train-mode BatchNorm: the batch mean absorbs them, so their
    exact gradient is ZERO and what a backward pass returns for them is rounding noise"""
    from gsn_amd.layers import mlp
    names = set()
    for name, m in model.named_modules():
        if isinstance(m, mlp) and m.batch_norm:
            names.update("%s.fc.%d.bias" % (name, i) for i in range(len(m.bn)))
    for i, conv in enumerate(model.conv):
        if model.bn[i]:
            names.add("conv.%d.update_fn.fc.%d.bias" % (i, len(conv.update_fn.fc) - 1))
    return names


LR, BETAS = 3e-4, (0.9, 0.999)          # (tests/test_graphed_train_gpu.py: larger steps amplify the atomics' last-bit noise)


def _adam_at(model):
    from gsn_amd.optim import Adam
    return Adam(model.parameters(), lr=LR, betas=BETAS)


def _eager_epoch(model, state0, graphs, kind, reverse=False):
    """the state after ONE eager epoch over the unpadded batches from ``state0``; ``reverse``: the graphs of every batch in reverse order --
    the same sets of graphs, hence the same step up to summation order, with every sum over vertices, edges and graphs taken in another order"""
    from gsn_amd import evaluation as ev
    model.load_state_dict(state0)
    model.train()
    opt = _adam_at(model)
    for idx in batches_of(len(graphs), B):
        data = _unpadded(graphs, idx[::-1] if reverse else idx)
        opt.zero_grad(set_to_none=True)
        ev.masked_loss(kind, model(data), data.y).backward()
        opt.step()
    torch.cuda.synchronize()
    model.eval()
    return _snapshot(model)


def _l2(a, b, keys):
    return float(sum(float((a[k].double() - b[k].double()).pow(2).sum()) for k in keys)) ** 0.5


def _check_epoch(tag, model, graphs, kind, state0, got):
    """``got`` (the state after one epoch through PaddedTrainStep from ``state0``) against the eager epoch over the unpadded batches.

    1. The project's measure over the whole state (tests/test_graphed_train_gpu.py: _rel), diff <= max(16 noise, 2e-5).  ``noise`` is the
       difference between eager unpadded runs from the same state: the larger of a repeated run and a run with the graphs of every batch in
       reverse order.  The feature promises equality UP TO SUMMATION ORDER, so the noise that belongs beside it is what a change of summation
       order does to the eager loop itself; a repeated run alone can reproduce its own rounding on these small shapes (measured: 6e-10 in
       some runs, 6e-4 in others), and then says nothing about order.
    2. Under Adam that noise is large (1e-3 .. 4e-3 after 3 steps) and figure 1 alone would pass a replay that never ran the optimizer.  Why:
       a Linear bias whose output goes straight into a train-mode BatchNorm has a gradient of exactly zero, the backward returns rounding
       noise for it, and Adam normalises noise to steps of the learning rate.  So the parameters are split.
       (a) The biases in front of a BatchNorm: no run can say where they go, but Adam bounds how far: |step| <= lr (1 - b1) / sqrt(1 - b2)
           per step (Kingma & Ba, section 2.1, the case 1 - b1 > sqrt(1 - b2)), so two runs differ by at most twice that times the steps.
       (b) Every other parameter, as ONE vector: the L2 distance between the replayed and the eager run, in units of the distance the eager
           run TRAVELLED from state0, held to the project's bar in the same units: max(16 x the distance of the reverse-order eager run,
           2e-5).  This is well conditioned (measured: 1.3e-6 .. 1.5e-6 replayed, 1.5e-6 .. 1.6e-6 reverse order).  An element's Adam step
           is about lr whatever its gradient's size, so a replay that took one step too few or too many out of 3, or never stepped, is
           off by a third of the travel or more, and a step counter or moment that the capture put back wrong rescales every step: all
           of that is four orders of magnitude above the bar.
    3. Every parameter the eager loop moved has moved, and integer state (num_batches_tracked) is equal (inside _rel)."""
    want, want2 = _eager_epoch(model, state0, graphs, kind), _eager_epoch(model, state0, graphs, kind)
    want_rev = _eager_epoch(model, state0, graphs, kind, reverse=True)
    n_steps = len(batches_of(len(graphs), B))
    noise = max(_rel(want, want2), _rel(want, want_rev))
    diff = _rel(want, got)
    where = _rel.where
    bar = max(16.0 * noise, 2e-5)
    zero = _biases_in_front_of_batchnorm(model)
    params = [k for k, _ in model.named_parameters()]
    assert zero <= set(params), sorted(zero - set(params))
    rest = [k for k in params if k not in zero]
    travel, err, err_rev = _l2(want, state0, rest), _l2(want, got, rest), _l2(want, want_rev, rest)
    step_cap = LR * (1.0 - BETAS[0]) / (1.0 - BETAS[1]) ** 0.5
    bias_far = max(float((want[k].double() - got[k].double()).abs().max()) for k in zero)
    print("padded-train epoch %s: whole state %.3g at %s, eager noise %.3g (bar %.3g)" % (tag, diff, where, noise, bar))
    print("padded-train epoch %s: parameters with a gradient: |replayed - eager| = %.3g of the travel %.3g (eager in reverse order: %.3g)"
          % (tag, err / travel, travel, err_rev / travel))
    print("padded-train epoch %s: biases in front of a BatchNorm differ by at most %.3g, Adam's bound for %d steps twice over is %.3g"
          % (tag, bias_far, n_steps, 2.0 * n_steps * step_cap))
    assert diff <= bar, "replayed epoch drifts from the eager unpadded loop: %.3g at %s (bar %.3g)" % (diff, where, bar)
    stuck = [k for k in params if _l2(want, state0, [k]) > 0.0 and not _l2(got, state0, [k]) > 0.0]
    assert travel > 0.0 and not stuck, "parameters the eager loop moved and the replays did not: %s" % stuck
    assert err / travel <= max(16.0 * err_rev / travel, 2e-5), ("replayed parameters are %.3g of the travelled distance away from the eager "
                                                                "loop's (reverse-order eager run: %.3g)" % (err / travel, err_rev / travel))
    assert bias_far <= 2.0 * n_steps * step_cap * (1.0 + 1e-3), "a zero-gradient bias moved further than Adam's steps allow: %.3g" % bias_far


@pytest.mark.parametrize("which", ["zinc", "ogb"])
def test_epochs_under_replay_follow_the_eager_unpadded_loop(which):
    """One epoch (3 batches) of PaddedTrainStep.run_epoch() with gsn_amd.optim.Adam at lr 3e-4 against the eager loop over the unpadded
    batches from the same state (_check_epoch says what is asserted and why); one capture, one replay per batch, a second epoch re-captures
    nothing."""
    from gsn_amd.graphs import PaddedTrainStep
    from gsn_amd.loader import PaddedDataLoader
    graphs, model, kind = _setup(which)
    if which == "ogb":
        graphs = molhiv_graphs(30, False)          # three batches: 12, 12 and 6 graphs
    n_batches = len(batches_of(len(graphs), B))
    assert n_batches == 3
    state0 = _snapshot(model)
    model.train()
    step = PaddedTrainStep(model, PaddedDataLoader(graphs, batch_size=B), kind, _adam_at(model))
    losses = step.run_epoch()
    assert losses.shape == (n_batches,) and bool(torch.isfinite(losses).all())
    assert (step.captures, step.replays, step.eager_batches) == (1, n_batches, 0)
    torch.cuda.synchronize()
    got = _snapshot(model)
    step.run_epoch()
    assert (step.captures, step.replays, step.eager_batches) == (1, 2 * n_batches, 0), "a second epoch re-captured"
    torch.cuda.synchronize()
    model.eval()
    _check_epoch(which, model, graphs, kind, state0, got)
    model.load_state_dict(state0)


def test_a_batch_that_does_not_fit_takes_an_eager_step():
    from gsn_amd.graphs import PaddedTrainStep
    from gsn_amd.loader import PaddedDataLoader
    graphs, model, kind = _setup("zinc")
    e = [int(g.edge_index.shape[1]) for g in graphs]
    per_batch = sorted(sum(e[i:i + B]) for i in (0, B))          # the two full batches; the larger one misses the capacity
    assert per_batch[0] < per_batch[1]
    state0 = _snapshot(model)
    model.train()
    step = PaddedTrainStep(model, PaddedDataLoader(graphs, batch_size=B, edge_capacity=per_batch[0]), kind, _adam_at(model))
    step.run_epoch()
    assert step.captures == 1 and step.eager_batches >= 1 and step.replays + step.eager_batches == 3
    torch.cuda.synchronize()
    model.eval()
    _check_epoch("zinc, one batch eager", model, graphs, kind, state0, _snapshot(model))
    model.load_state_dict(state0)


def test_refusals():
    """one real graph in front of GNN_OGB's virtual-node BatchNorm: torch's ValueError, from host numbers, before any replay; a padded batch in
    training mode outside the opt-in still raises; a plain DataLoader is a TypeError"""
    from gsn_amd.graphs import PaddedTrainStep
    from gsn_amd.loader import DataLoader, PaddedDataLoader, masked_training
    graphs, model = molhiv_graphs(), ogb_model()                    # 25 graphs: batches of 12, 12 and ONE (single-vertex) graph
    state0 = _snapshot(model)
    loader = PaddedDataLoader(graphs, batch_size=B)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model(next(iter(loader)))
    for batch in loader:                                            # (run the iterator out: one live iterator per padded loader)
        pass
    assert batch.num_real_graphs == 1
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        with masked_training(batch):
            model(batch)
    step = PaddedTrainStep(model, loader, "BCEWithLogitsLoss", _adam_at(model))
    it = iter(loader)
    step.step(next(it)); step.step(next(it))
    assert (step.captures, step.replays) == (1, 2)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        step.step(next(it))
    assert (step.captures, step.replays, step.eager_batches) == (1, 2, 0)
    with pytest.raises(TypeError, match="PaddedDataLoader"):
        PaddedTrainStep(model, DataLoader(graphs, batch_size=B), "BCEWithLogitsLoss", _adam_at(model))
    model.eval()
    with pytest.raises(RuntimeError, match="evaluation mode"):
        step.step(batch)
    model.load_state_dict(state0)
