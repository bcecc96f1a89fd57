"""Counted accumulation on the GPU (gsn_eval_accumulate_counted_hip, EpochAccumulator.add(..., n_valid=...)): with v = clamp(n_valid, 0, rows)
read on the device it must do exactly what gsn_eval_accumulate_hip does when called with rows = v, num_graphs = v on the same pointers --
the accumulator words, the appended rows and last_loss are compared BIT FOR BIT, with rows >= v poisoned (NaN, infinities, classes out of
range), on accumulators that already hold a batch.  Across the two-launch switch the host `rows` picks the launch path: where the two calls
take different paths the loss is compared with the float64 referee tests/eval_ref.py within the bar of tests/test_evaluation_gpu.py."""
import numpy as np
import pytest
import torch

from eval_ref import masked_loss_ref, normalised_error
from gsn_amd import evaluation as ev
from gsn_amd.graphs import GraphedStep

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR = 2.0 ** -22            # the floor of tests/test_evaluation_gpu.py's bar
CASES = [("BCEWithLogitsLoss", None), ("L1Loss", "L1Loss"), ("MSELoss", "MSELoss"), ("L1Loss", "MSELoss"), ("CrossEntropyLoss", "multi_class_accuracy"),
         ("CrossEntropyLoss", None)]


def _inputs(kind, rows, cols, seed, v=None):
    """device tensors; rows >= v poisoned"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 3
    if kind == "CrossEntropyLoss":
        y = torch.randint(0, cols, (rows,), generator=g)
    else:
        y = torch.randint(0, 2, (rows, cols), generator=g).float() if kind == "BCEWithLogitsLoss" else torch.randn(rows, cols, generator=g)
        y.view(-1)[torch.rand(rows * cols, generator=g) < 0.25] = float("nan")
    if v is not None and v < rows:
        x[v:] = float("nan")
        x[v::2] = float("inf")
        x[v::3] = -float("inf")
        if kind == "CrossEntropyLoss":
            y[v:] = 99
            y[v::2] = -5
        else:
            y[v:] = float("inf")
            y[v::2] = -1e30
    return x.to(DEV), y.to(DEV)


def _acc(kind, metric, cap, cols):
    acc = ev.EpochAccumulator(cap, cols, cols, kind, metric, device=DEV)
    acc.y_pred.fill_(-7.0)
    acc.y_true.fill_(-7)
    return acc


def _nv(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _same(a, b, what):
    assert torch.equal(a._state.cpu(), b._state.cpu()), (what, a._state.cpu().tolist(), b._state.cpu().tolist())
    assert torch.equal(a.last_loss.view(torch.int32).cpu(), b.last_loss.view(torch.int32).cpu()), what
    assert torch.equal(a.y_pred.view(torch.int32).cpu(), b.y_pred.view(torch.int32).cpu()), what
    pt = torch.int64 if a.y_true.dtype == torch.int64 else torch.int32
    assert torch.equal(a.y_true.view(pt).cpu(), b.y_true.view(pt).cpu()), what


@pytest.mark.parametrize("rows", [5, 1030])
@pytest.mark.parametrize("kind,metric", CASES)
def test_counted_equals_the_call_on_the_valid_rows_bit_for_bit(kind, metric, rows):
    cols = 4 if kind == "CrossEntropyLoss" else 3
    x0, y0 = _inputs(kind, 7, cols, 1)                      # a batch both accumulators already hold
    for v in (0, 1, rows - 1, rows, rows + 5, -3):
        x, y = _inputs(kind, rows, cols, 10 + rows, v=max(min(v, rows), 0))
        a, b = _acc(kind, metric, rows + 16, cols), _acc(kind, metric, rows + 16, cols)
        a.add(x0, y0, 7)
        b.add(x0, y0, 7)
        a.add(x, y, n_valid=_nv(v))
        w = max(min(v, rows), 0)
        b.add(x[:w], y[:w], num_graphs=w)                  # (a prefix view: the same pointers)
        _same(a, b, (kind, metric, rows, v))
        st = a._state.cpu()
        assert st[4:].tolist()[:2] == [7 + w, 2 if w else 1] and int(st[7]) == 0
        assert bool((a.y_pred[7 + w:] == -7.0).all()) and bool((a.y_true[7 + w:] == -7).all())
        if w:
            assert bool(torch.isfinite(a.last_loss)) or kind != "CrossEntropyLoss"
    # an overflowing counted batch changes nothing but the status word, as the ordinary call
    x, y = _inputs(kind, rows, cols, 3)
    a, b = _acc(kind, metric, rows + 6, cols), _acc(kind, metric, rows + 6, cols)
    for acc in (a, b):
        acc.add(x0, y0, 7)
    a.add(x, y, n_valid=_nv(rows))
    b.add(x, y, num_graphs=rows)
    _same(a, b, (kind, metric, rows, "overflow"))
    assert a._state.cpu()[4:].tolist() == [7, 1, b._state.cpu()[6].item(), 1]
    with pytest.raises(TypeError):
        a.add(x, y, n_valid=3)
    with pytest.raises(TypeError):
        a.add(x, y, n_valid=torch.tensor([3], dtype=torch.int32, device=DEV))


def test_across_the_two_launch_switch():
    """rows = 65 537, one column: the host picks the partial + combine launches.  v = 65 537: the ordinary call takes them too -- bit for bit.
    v = 100: the ordinary call on 100 rows is one launch -- against the float64 referee, and the appended rows exactly."""
    rows, kind = 65537, "BCEWithLogitsLoss"
    for metric_kind, metric in ((kind, None), ("L1Loss", "L1Loss")):
        x, y = _inputs(metric_kind, rows, 1, 21)
        a, b = _acc(metric_kind, metric, rows + 8, 1), _acc(metric_kind, metric, rows + 8, 1)
        a.add(x, y, n_valid=_nv(rows))
        b.add(x, y, num_graphs=rows)
        _same(a, b, (metric_kind, "v = rows"))
        assert a._state.cpu()[4:].tolist()[:2] == [rows, 1]
    v = 100
    x, y = _inputs(kind, rows, 1, 22, v=v)
    a = _acc(kind, None, rows + 8, 1)
    a.add(x, y, n_valid=_nv(v))
    st = a._state.cpu()
    loss = float(a.last_loss)
    assert st[4:].tolist() == [v, 1, 0, 0]
    assert st[:4].view(torch.float64).tolist()[:2] == [loss * v, loss]
    assert torch.equal(a.y_pred[:v].view(torch.int32), x[:v].view(torch.int32)) and torch.equal(a.y_true[:v].view(torch.int32), y[:v].view(torch.int32))
    assert bool((a.y_pred[v:] == -7.0).all()) and bool((a.y_true[v:] == -7.0).all())
    xc, yc = x[:v].cpu(), y[:v].cpu()
    ref, scale, _, _ = masked_loss_ref(kind, xc.numpy(), yc.numpy(), 1.0)
    lab = yc == yc
    tor = torch.nn.BCEWithLogitsLoss()(xc[lab], yc[lab])
    bar = max(2.0 * normalised_error(tor.numpy(), ref, scale), FLOOR)
    err = normalised_error(np.float32(loss), ref, scale)
    print("two-launch path on 100 valid rows: normalised loss error %.3g, bar %.3g" % (err, bar))
    assert err <= bar, (err, bar)


def test_a_replayed_add_appends_exactly_the_valid_rows():
    rows, cols, kind = 64, 3, "BCEWithLogitsLoss"
    sx, sy, nv = torch.zeros(rows, cols, device=DEV), torch.zeros(rows, cols, device=DEV), _nv(rows)
    counts = (64, 0, 1, 63, 17, 64, 0)
    a, b = _acc(kind, "L1Loss", sum(counts) + 4, cols), _acc(kind, "L1Loss", sum(counts) + 4, cols)
    step = GraphedStep(lambda: a.add(sx, sy, n_valid=nv))
    a.reset()                                              # (the warm-up runs were real calls)
    a.y_pred.fill_(-7.0)
    a.y_true.fill_(-7.0)
    a.last_loss.zero_()
    xs, ys = [], []
    for r, v in enumerate(counts):
        x, y = _inputs(kind, rows, cols, 40 + r, v=v)
        sx.copy_(x)
        sy.copy_(y)
        nv.fill_(v)
        step()
        b.add(x[:v], y[:v], num_graphs=v)
        xs.append(x[:v])
        ys.append(y[:v])
    _same(a, b, "replays")
    res = a.result()
    assert res.n_rows == sum(counts) and res.n_batches == sum(1 for v in counts if v)
    assert torch.equal(res.y_pred.view(torch.int32), torch.cat(xs).view(torch.int32)) and torch.equal(res.y_true.view(torch.int32), torch.cat(ys).view(torch.int32))
