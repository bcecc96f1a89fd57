"""Device-side evaluation on the GPU (gsn_amd/evaluation.py, csrc/evaluate.hip) against the float64 / exact-integer referee tests/eval_ref.py.

The bar of every loss and gradient comparison is computed by the test, as in test_optim_gpu.py: the normalised error of torch's own fp32
evaluation (CPU) of the reference's expression ``loss_fn(y_hat[is_labeled], y[is_labeled])`` on the SAME inputs, times 2, and never below
2^-22.  Rank statistics are integers and must be equal; auc is one correctly rounded division of them and must be equal; ap is within 1e-12
(a float64 sum of at most M terms of total <= 1 in another order)."""
import math

import numpy as np
import pytest
import torch

from eval_ref import FP32_TINY, KINDS, masked_loss_ref, normalised_error, rank_ref
from gsn_amd import evaluation as ev
from gsn_amd.graphs import GraphedStep

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
DEV = "cuda"
TORCH_LOSS = {"BCEWithLogitsLoss": torch.nn.BCEWithLogitsLoss, "L1Loss": torch.nn.L1Loss, "MSELoss": torch.nn.MSELoss,
              "CrossEntropyLoss": torch.nn.CrossEntropyLoss}
# rows per T: element counts 1, 63, 64, 65, 1 023, 1 024, 1 025, 2 049, 65 536, 65 537, 70 001 -- for T = 3 / 128 the row counts whose element
# counts lie on both sides of a chunk (1 024) and of the one-launch limit (65 536)
SHAPES = [(n, 1) for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 65536, 65537, 70001)]
SHAPES += [(r, 3) for r in (1, 21, 341, 342, 683, 21845, 21846, 23334)] + [(r, 128) for r in (1, 8, 9, 512, 513, 547)]


def _inputs(kind, rows, cols, share, seed):
    """fp32 CPU tensors: logits up to +-100 with +-0 among them, targets with a `share` of NaN ('one': all but one, 'all')"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 4
    n = rows * cols
    flat = x.view(-1)
    for i, v in enumerate((100.0, -100.0, 0.0, -0.0, 99.5, -87.0)):
        if n > i + 1:
            flat[(i * 7919 + 1) % n] = v
    if kind == "BCEWithLogitsLoss":
        y = torch.randint(0, 2, (rows, cols), generator=g).float()
    else:
        y = torch.randn(rows, cols, generator=g) * 3
    m = torch.zeros(n, dtype=torch.bool)
    if share == "all":
        m[:] = True
    elif share == "one":
        m[:] = True
        m[n // 2] = False
    elif share:
        m = torch.rand(n, generator=g) < share
    y.view(-1)[m] = float("nan")
    return x, y


def _torch_masked(kind, x, y, upstream):
    """torch's fp32 evaluation of train_test_funcs.py:98-101 on the CPU: (loss, grad)"""
    x = x.clone().requires_grad_(True)
    lab = y == y
    loss = TORCH_LOSS[kind]()(x[lab], y[lab])
    (loss * upstream).backward()
    return loss.detach(), x.grad


def _native(kind, x, y, upstream):
    xd = x.to(DEV).requires_grad_(True)
    loss, count = ev.masked_loss(kind, xd, y.to(DEV), return_count=True)
    (loss * upstream).backward()
    return loss.detach(), xd.grad, count


def _check(kind, x, y, upstream, what, worst):
    ref, scale, gref, gscale = masked_loss_ref(kind, x.numpy(), y.numpy(), upstream)
    loss, grad, count = _native(kind, x, y, upstream)
    labelled = int((y == y).sum()) if kind != "CrossEntropyLoss" else x.shape[0]
    assert int(count) == labelled, what
    if labelled == 0:
        assert math.isnan(float(loss)) and not grad.any(), what
        return
    tl, tg = _torch_masked(kind, x, y, upstream)
    bars = (max(2.0 * normalised_error(tl.numpy(), ref, scale), FLOOR), max(2.0 * normalised_error(tg.numpy(), gref, gscale, FP32_TINY), FLOOR))
    errs = (normalised_error(loss.cpu().numpy(), ref, scale), normalised_error(grad.cpu().numpy(), gref, gscale, FP32_TINY))
    worst[0], worst[1] = max(worst[0], errs[0] / bars[0]), max(worst[1], errs[1] / bars[1])
    assert math.isfinite(float(loss)), what
    assert errs[0] <= bars[0] and errs[1] <= bars[1], "%s: loss off by %.3g (bar %.3g), gradient by %.3g (bar %.3g)" % (what, errs[0], bars[0], errs[1], bars[1])
    if kind != "CrossEntropyLoss":
        assert not grad.cpu()[(y != y).view(grad.shape)].any(), what      # zeros at unlabelled positions


@pytest.mark.parametrize("kind", KINDS[:3])
def test_masked_loss_and_gradient_against_referee(kind):
    worst = [0.0, 0.0]
    for rows, cols in SHAPES:
        for s, share in enumerate((0, 0.3, "one", "all")):
            x, y = _inputs(kind, rows, cols, share, 1000 * rows + 10 * cols + s)
            _check(kind, x, y, 1.0 if s % 2 == 0 else -3.5, "%s %dx%d NaN %s" % (kind, rows, cols, share), worst)
    print("%s: worst error / bar: loss %.3f gradient %.3f" % (kind, worst[0], worst[1]))


def test_targets_are_viewed_to_the_predictions_shape():
    x, y = _inputs("BCEWithLogitsLoss", 65, 1, 0.3, 3)
    a = ev.masked_loss("BCEWithLogitsLoss", x.to(DEV), y.to(DEV))
    b = ev.masked_loss("BCEWithLogitsLoss", x.to(DEV), y.view(-1).to(DEV))                   # [B] against [B, 1]
    c = ev.MaskedLoss("BCEWithLogitsLoss")(x.view(-1).to(DEV), y.to(DEV))
    assert a.shape == () and torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(TypeError):
        ev.masked_loss("BCEWithLogitsLoss", x.double().to(DEV), y.to(DEV))
    with pytest.raises(ValueError):
        ev.masked_loss("BCEWithLogitsLoss", x.to(DEV), y[:-1].to(DEV))
    with pytest.raises(NotImplementedError):
        ev.masked_loss("HuberLoss", x.to(DEV), y.to(DEV))


@pytest.mark.parametrize("n_cls", [2, 37])
def test_cross_entropy_against_referee(n_cls):
    worst = [0.0, 0.0]
    for rows in (1, 65, 1025, 1771 if n_cls == 37 else 32769):              # the last: beyond the one-launch limit
        g = torch.Generator().manual_seed(rows + n_cls)
        x = torch.randn(rows, n_cls, generator=g) * 6
        x[0, 0], x[0, 1] = 100.0, -100.0
        t = torch.randint(0, n_cls, (rows,), generator=g)
        _check("CrossEntropyLoss", x, t, 1.0 if rows % 2 else 0.25, "CE %dx%d" % (rows, n_cls), worst)
        if rows >= 65:          # a target outside the classes: NaN loss, that row's gradient zero, the other rows as without it; no fault
            bad = t.clone()
            bad[3], bad[40] = n_cls, -1
            ref, scale, gref, gscale = masked_loss_ref("CrossEntropyLoss", x.numpy(), bad.numpy())
            loss, grad, count = _native("CrossEntropyLoss", x, bad, 1.0)
            assert math.isnan(float(loss)) and math.isnan(ref) and int(count) == rows
            assert not grad[3].any() and not grad[40].any()
            assert normalised_error(grad.cpu().numpy(), gref, gscale, FP32_TINY) <= FLOOR
    print("CrossEntropyLoss C = %d: worst error / bar: loss %.3f gradient %.3f" % (n_cls, worst[0], worst[1]))


def _acc_for(kind, cap, cols, metric=None):
    return ev.EpochAccumulator(cap, cols, cols, kind, metric, device=DEV)


@pytest.mark.parametrize("shape", [(65, 3), (1025, 1), (70001, 1), (547, 128)])
def test_two_runs_and_the_accumulator_give_the_same_bits(shape):
    rows, cols = shape
    for kind in KINDS[:3]:
        x, y = _inputs(kind, rows, cols, 0.3, 5)
        l1, g1, _ = _native(kind, x, y, 1.0)
        l2, g2, _ = _native(kind, x, y, 1.0)
        assert l1.view(torch.int32).item() == l2.view(torch.int32).item() and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
        acc = _acc_for(kind, rows, cols)
        acc.add(x.to(DEV), y.to(DEV))
        assert acc.last_loss.view(torch.int32).item() == l1.view(torch.int32).item(), kind
    x = torch.randn(rows, max(cols, 2))
    t = torch.randint(0, max(cols, 2), (rows,))
    l1, _, _ = _native("CrossEntropyLoss", x, t, 1.0)
    acc = _acc_for("CrossEntropyLoss", rows, max(cols, 2))
    acc.add(x.to(DEV), t.to(DEV))
    assert acc.last_loss.view(torch.int32).item() == l1.view(torch.int32).item()


def test_masked_loss_replays_in_a_captured_graph():
    """GraphedStep over masked_loss + autograd.grad with respect to a static y_hat; y is refilled between replays, so the NaN positions and the
    labelled count change.  Every replay equals the eager result bit for bit."""
    rows, cols = 128, 3
    sx = torch.zeros(rows, cols, device=DEV, requires_grad=True)
    sy = torch.zeros(rows, cols, device=DEV)

    def fn():
        loss, count = ev.masked_loss("BCEWithLogitsLoss", sx, sy, return_count=True)
        (grad,) = torch.autograd.grad(loss, sx)
        return loss, grad, count

    x0, y0 = _inputs("BCEWithLogitsLoss", rows, cols, 0.5, 0)
    with torch.no_grad():
        sx.copy_(x0)
    sy.copy_(y0)
    step = GraphedStep(fn)
    counts = set()
    for r, share in enumerate((0.1, 0.6, "one", "all", 0)):
        x, y = _inputs("BCEWithLogitsLoss", rows, cols, share, 50 + r)
        with torch.no_grad():
            sx.copy_(x)
        sy.copy_(y)
        loss, grad, count = step()
        el, eg, ec = _native("BCEWithLogitsLoss", x, y, 1.0)
        assert int(count) == int(ec) == int((y == y).sum())
        assert torch.equal(loss.view(torch.int32), el.view(torch.int32)) and torch.equal(grad.view(torch.int32), eg.view(torch.int32)), share
        counts.add(int(count))
    assert len(counts) == 5 and 0 in counts


def test_accumulator_appends_in_a_captured_graph():
    rows, cols = 64, 3
    sx = torch.zeros(rows, cols, device=DEV)
    sy = torch.zeros(rows, cols, device=DEV)
    acc = _acc_for("BCEWithLogitsLoss", 3 * rows, cols)
    sx.copy_(_inputs("BCEWithLogitsLoss", rows, cols, 0.3, 1)[0])
    step = GraphedStep(lambda: acc.add(sx, sy))
    acc.reset()                                   # (the warm-up runs were real calls)
    xs, ys, want = [], [], 0.0
    for r in range(3):
        x, y = _inputs("BCEWithLogitsLoss", rows, cols, 0.2 * r, 70 + r)
        sx.copy_(x)
        sy.copy_(y)
        step()
        xs.append(x)
        ys.append(y)
        want += float(ev.masked_loss("BCEWithLogitsLoss", x.to(DEV), y.to(DEV))) * rows
    res = acc.result()
    assert res.n_rows == 3 * rows and res.n_batches == 3 and res.weighted_loss_sum == want
    assert torch.equal(res.y_pred.cpu().view(torch.int32), torch.cat(xs).view(torch.int32))
    assert torch.equal(res.y_true.cpu().view(torch.int32), torch.cat(ys).view(torch.int32))


def test_accumulator_sums_rows_and_overflow():
    cols, sizes = 3, (1, 64, 37, 128, 1)
    cap = sum(sizes)
    acc = _acc_for("BCEWithLogitsLoss", cap, cols)
    xs, ys, weighted, plain = [], [], 0.0, 0.0
    for b, rows in enumerate(sizes):
        x, y = _inputs("BCEWithLogitsLoss", rows, cols, 0.3 if rows > 1 else 0, 200 + b)
        acc.add(x.to(DEV), y.to(DEV), num_graphs=rows)
        l = float(ev.masked_loss("BCEWithLogitsLoss", x.to(DEV), y.to(DEV)))
        weighted += l * rows
        plain += l
        xs.append(x)
        ys.append(y)
    r = acc.result()
    assert (r.n_rows, r.n_batches) == (cap, len(sizes)) and r.weighted_loss_sum == weighted and r.batch_loss_sum == plain and r.metric_sum == 0.0
    assert torch.equal(r.y_pred.cpu().view(torch.int32), torch.cat(xs).view(torch.int32))
    assert torch.equal(r.y_true.cpu().view(torch.int32), torch.cat(ys).view(torch.int32))
    acc.reset()
    assert acc.result().n_rows == 0 and acc.result().weighted_loss_sum == 0.0
    # overflow: the batch that would pass the capacity writes nothing, result() raises; sentinel rows behind the buffers stay
    cap = 100
    acc = _acc_for("BCEWithLogitsLoss", cap, cols)
    big_p = torch.full((cap + 8, cols), -7.0, device=DEV)
    big_t = torch.full((cap + 8, cols), -7.0, device=DEV)
    acc.y_pred, acc.y_true = big_p[:cap], big_t[:cap]
    acc.add(xs[1].to(DEV), ys[1].to(DEV))
    acc.add(xs[3].to(DEV), ys[3].to(DEV))          # 64 + 128 > 100
    acc.add(xs[2].to(DEV), ys[2].to(DEV))          # 64 + 37 > 100 as well: the flag stays, nothing moves
    with pytest.raises(RuntimeError, match="did not fit"):
        acc.result()
    assert torch.equal(big_p[:64].cpu(), xs[1]) and bool((big_p[64:] == -7.0).all()) and bool((big_t[64:] == -7.0).all())
    assert acc._state.cpu()[4:].tolist() == [64, 1, 0, 1]
    # the same on the two-launch path (more than 65 536 elements: the partial pass returns early, the combine pass sets the flag)
    rows, cap = 70001, 70001 + 10
    x, y = _inputs("BCEWithLogitsLoss", rows, 1, 0.3, 9)
    acc = _acc_for("BCEWithLogitsLoss", cap, 1)
    big_p = torch.full((cap + 8, 1), -7.0, device=DEV)
    big_t = torch.full((cap + 8, 1), -7.0, device=DEV)
    acc.y_pred, acc.y_true = big_p[:cap], big_t[:cap]
    acc.add(x.to(DEV), y.to(DEV))
    first = acc._state.cpu().clone()
    acc.add(y.to(DEV), x.to(DEV))                  # 2 x 70 001 > 70 011
    with pytest.raises(RuntimeError, match="did not fit"):
        acc.result()
    assert torch.equal(big_p[:rows].cpu().view(torch.int32), x.view(torch.int32)) and bool((big_p[rows:] == -7.0).all()) and bool((big_t[rows:] == -7.0).all())
    after = acc._state.cpu()
    assert after[4:].tolist() == [rows, 1, 0, 1] and torch.equal(after[:4], first[:4])          # the sums did not move either


def test_empty_shapes():
    """No element: the mean of nothing is NaN, the count 0 and the gradient empty, as torch; nothing is read.  CrossEntropyLoss rows without a
    class column are refused before any launch (no target class and no maximum to read)."""
    for kind, shape in (("BCEWithLogitsLoss", (0, 3)), ("L1Loss", (5, 0)), ("MSELoss", (0,))):
        x = torch.empty(shape, device=DEV, requires_grad=True)
        loss, count = ev.masked_loss(kind, x, torch.empty(shape, device=DEV), return_count=True)
        loss.backward()
        assert math.isnan(float(loss.detach())) and int(count) == 0 and x.grad.shape == x.shape, kind
    x = torch.empty((0, 5), device=DEV, requires_grad=True)
    loss, count = ev.masked_loss("CrossEntropyLoss", x, torch.empty(0, dtype=torch.int64, device=DEV), return_count=True)
    loss.backward()
    assert math.isnan(float(loss.detach())) and int(count) == 0
    t = torch.zeros(5, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="at least one class"):
        ev.masked_loss("CrossEntropyLoss", torch.empty((5, 0), device=DEV), t)
    with pytest.raises(ValueError, match="at least one class"):
        ev.EpochAccumulator(8, 0, 1, "CrossEntropyLoss", device=DEV).add(torch.empty((5, 0), device=DEV), t)
    # the entry itself, with somewhere to write and a null prediction pointer (a 0-element tensor's): refused, nothing launched
    from gsn_amd import _abi
    out = torch.full((2,), 3.0, device=DEV)
    cnt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    rc = _abi.lib().gsn_masked_loss_fwd_hip(3, 5, 0, None, t.data_ptr(), out.data_ptr(), cnt.data_ptr(), None, 0, _abi.current_stream())
    assert rc == -1 and out.tolist() == [3.0, 3.0] and int(cnt) == 7


@pytest.mark.parametrize("rows", [37, 70001])
def test_accumulator_metric_terms(rows):
    """L1 / MSE sums (fp32 reduction='sum' per batch, added in float64) and the arg-max count, on both launch paths"""
    g = torch.Generator().manual_seed(rows)
    x, y = torch.randn(rows, 1, generator=g), torch.randn(rows, 1, generator=g)
    for metric, f in (("L1Loss", lambda d: d.abs()), ("MSELoss", lambda d: d * d)):
        acc = ev.EpochAccumulator(0, 1, 1, "L1Loss", metric, device=DEV, keep_rows=False)
        acc.add(x.to(DEV), y.to(DEV))
        acc.add(y.to(DEV), x.to(DEV))
        exact = float(f(x.double() - y.double()).sum())
        got = acc.result().metric_sum
        # The metric is DEFINED as an fp32 number per batch (utils.py:177-183: reduction='sum' of fp32 terms), so it is not "exact or within
        # 1e-12" of a float64 sum; it is within ONE fp32 ulp of that sum rounded to fp32: the terms are rounded to fp32 (2^-24 relative each,
        # all positive, so < 1 ulp of the sum together), added in float64 and rounded once more -- two roundings of values < 1 ulp apart.
        assert abs(got / 2 - float(np.float32(exact))) <= float(np.spacing(np.float32(exact))), metric
        assert float(ev.prediction_function(metric)(x.to(DEV), y.to(DEV))) == float(np.float32(got / 2))
    n_cls = 7
    x = torch.randn(rows, n_cls, generator=g)
    x[5] = 1.0                                      # a row of ties: the first index
    t = torch.randint(0, n_cls, (rows,), generator=g)
    acc = ev.EpochAccumulator(0, n_cls, 1, torch.nn.CrossEntropyLoss(), "multi_class_accuracy", device=DEV, keep_rows=False)
    acc.add(x.to(DEV), t.to(DEV))
    want = int((x.argmax(1) == t).sum())
    assert acc.result().metric_sum == want and float(ev.prediction_function("multi_class_accuracy")(x.to(DEV), t.to(DEV))) == want
    with pytest.raises(ValueError):
        ev.EpochAccumulator(0, 1, 1, "L1Loss", "multi_class_accuracy", device=DEV)


def _tie_scores(m, rng):
    s = np.arange(m, dtype=np.float32)
    if m > 1100:
        s[1000:1101] = s[1000]
    if m > 4100:
        s[4090:4101] = s[4090]
    return s[rng.permutation(m)]


def _score_cases(m, rng):
    yield "random", rng.standard_normal(m).astype(np.float32)
    yield "all_equal", np.full(m, -1.5, dtype=np.float32)
    yield "tie_runs", _tie_scores(m, rng)
    d = np.float32(1e-45)
    yield "zeros_denormals", rng.choice(np.array([0.0, -0.0, d, -d, 2 * d, 1e-39, -1e-39, 1e-30], dtype=np.float32), size=m)
    yield "few_values", rng.integers(-2, 3, size=m).astype(np.float32)


@pytest.mark.parametrize("m", [2, 3, 4095, 4096, 4097, 8193, 12293])
def test_rank_metrics_against_referee(m):
    rng = np.random.default_rng(m)
    for name, s0 in _score_cases(m, rng):
        pred = np.stack([s0, rng.standard_normal(m).astype(np.float32), s0[::-1]], axis=1)
        true = np.stack([rng.integers(0, 2, size=m), np.ones(m), rng.integers(0, 2, size=m)], axis=1).astype(np.float32)
        true[0, 0], true[1, 0] = 0.0, 1.0                                # column 0 has both classes
        true[0, 2], true[1, 2] = 1.0, 0.0
        if m > 3:
            true[rng.random(m) < 0.3, 2] = np.nan                        # column 2 has unlabelled rows
            true[0, 2], true[1, 2] = 1.0, 0.0
        ints, floats, status = ev.rank_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(true).to(DEV))
        aucs, aps = [], []
        for c in range(3):
            r = rank_ref(pred[:, c], true[:, c])
            assert ints[c].tolist() == [r["n"], r["n_pos"], r["u2"]], (name, m, c)
            if c == 1:
                assert status[c] == ev.ST_ONE_CLASS and math.isnan(floats[c, 0])
            else:
                assert status[c] == 0
                assert floats[c, 0] == r["u2"] / (2 * r["n_pos"] * (r["n"] - r["n_pos"])) == r["auc"], (name, m, c)
                aucs.append(r["auc"])
            assert abs(floats[c, 1] - r["ap"]) <= 1e-12, (name, m, c)
            aps.append(r["ap"])
        inp = {"y_true": true, "y_pred": torch.from_numpy(pred).to(DEV)}          # a numpy array is uploaded
        assert ev.Evaluator("ogbg-molhiv").eval(inp) == {"rocauc": sum(aucs) / 2}
        assert abs(ev.Evaluator("ogbg-molpcba").eval(inp)["ap"] - sum(aps) / 3) <= 1e-12


def test_evaluator_refusals_and_acc():
    pred = np.array([[0.1, 0.2], [0.4, np.inf], [0.3, 0.5], [0.9, 0.1]], dtype=np.float32)
    true = np.array([[0, 1], [1, np.nan], [1, 0], [0, 1]], dtype=np.float32)
    e = ev.Evaluator("ogbg-molhiv")
    assert e.eval({"y_true": true, "y_pred": pred})["rocauc"] == (rank_ref(pred[:, 0], true[:, 0])["auc"] + rank_ref(pred[:, 1], true[:, 1])["auc"]) / 2
    bad = true.copy()
    bad[1, 1] = 1.0                                   # the infinite prediction is now in a labelled row
    with pytest.raises(ValueError, match="column 1 of y_pred"):
        e.eval({"y_true": bad, "y_pred": pred})
    bad = true.copy()
    bad[2, 0] = 2.0
    with pytest.raises(ValueError, match="column 0 of y_true"):
        e.eval({"y_true": bad, "y_pred": pred})
    with pytest.raises(RuntimeError, match="No positively labeled"):
        e.eval({"y_true": np.ones((4, 2), dtype=np.float32), "y_pred": pred[:, :1].repeat(2, axis=1)})
    with pytest.raises(RuntimeError, match="No positively labeled"):
        ev.Evaluator("ogbg-molpcba").eval({"y_true": np.zeros((4, 2), dtype=np.float32), "y_pred": pred[:, :1].repeat(2, axis=1)})
    with pytest.raises(RuntimeError):
        e.eval({"y_true": true, "y_pred": pred[:, :1]})
    yt = np.array([[1], [2], [3], [3]], dtype=np.int64)
    yp = np.array([[1], [0], [3], [3]], dtype=np.int64)
    assert ev.Evaluator("ogbg-ppa").eval({"y_true": yt, "y_pred": yp}) == {"acc": 0.75}


class _Batch:
    def __init__(self, feat, x, y):
        self.feat, self.x, self.y, self.num_graphs = feat, x, y, feat.shape[0]

    def to(self, device):
        return _Batch(self.feat.to(device), self.x.to(device), self.y.to(device))


class _Loader(list):
    """a list of batches with the two attributes the loops read"""

    def __init__(self, batches, dataset_len):
        super().__init__(batches)
        self.dataset = range(dataset_len)


class _Model(torch.nn.Module):
    def __init__(self, d_in, d_out):
        super().__init__()
        torch.manual_seed(0)
        self.lin = torch.nn.Linear(d_in, d_out)

    def forward(self, batch):
        return self.lin(batch.feat)


def _loss_bar(kind, preds, ys, weights, total):
    """(referee value, scale, torch's fp32 value) of  sum_b loss_b * w_b / total  over the batches"""
    ref = scale = tor = 0.0
    for p, y, w in zip(preds, ys, weights):
        r, s, _, _ = masked_loss_ref(kind, p.numpy(), y.numpy())
        lab = y == y if kind != "CrossEntropyLoss" else None
        t = TORCH_LOSS[kind]()(p[lab], y[lab]) if lab is not None else TORCH_LOSS[kind]()(p, y)
        ref, scale, tor = ref + r * w, scale + s * w, tor + t.item() * w
    return ref / total, scale / total, tor / total


def test_loops_against_the_reference_arithmetic():
    g = torch.Generator().manual_seed(9)
    sizes, d_in, n_tasks = (32, 32, 1, 17), 6, 3
    model = _Model(d_in, n_tasks).to(DEV)
    batches = []
    for b in sizes:
        y = torch.randint(0, 2, (b, n_tasks), generator=g).float()
        y[torch.rand(b, n_tasks, generator=g) < 0.25] = float("nan")
        y[:, 1] = 1.0 if b > 1 else y[:, 1]                                   # task 1 has one class in every real batch: skipped
        batches.append(_Batch(torch.randn(b, d_in, generator=g), torch.zeros(1 if b == 1 else 3 * b, 2), y))
    loader = _Loader(batches, sum(sizes))
    with torch.no_grad():
        preds = [model(bt.to(DEV)).cpu() for bt in batches]
    # test_ogb: the batch whose x has one row is skipped; rocauc over the non-skipped tasks
    kept = [i for i, b in enumerate(sizes) if b != 1]
    loss, metric = ev.test_ogb(loader, model, torch.nn.BCEWithLogitsLoss(), DEV, ev.Evaluator("ogbg-molhiv"))
    ref, scale, tor = _loss_bar("BCEWithLogitsLoss", [preds[i] for i in kept], [batches[i].y for i in kept], [sizes[i] for i in kept], sum(sizes))
    assert abs(loss - ref) / scale <= max(2.0 * abs(tor - ref) / scale, FLOOR)
    P, Y = torch.cat([preds[i] for i in kept]).numpy(), torch.cat([batches[i].y for i in kept]).numpy()
    aucs = [rank_ref(P[:, c], Y[:, c])["auc"] for c in range(n_tasks)]
    assert aucs[1] is None and metric == (aucs[0] + aucs[2]) / 2
    aps = [rank_ref(P[:, c], Y[:, c])["ap"] for c in range(n_tasks)]
    _, metric = ev.test_ogb(loader, model, ev.MaskedLoss("BCEWithLogitsLoss"), DEV, ev.Evaluator("ogbg-molpcba"))
    assert abs(metric - sum(aps) / 3) <= 1e-12

    class Foreign:                                                            # an evaluator that is not ours gets numpy arrays
        name, eval_metric = "ogbg-molhiv", "rows"

        def eval(self, d):
            assert isinstance(d["y_true"], np.ndarray) and isinstance(d["y_pred"], np.ndarray)
            return {"rows": d["y_pred"].shape[0]}
    assert ev.test_ogb(loader, model, "BCEWithLogitsLoss", DEV, Foreign())[1] == sum(sizes) - 1
    # n_iters beyond one pass: the loader restarts
    loss2, _ = ev.test_ogb(loader, model, "BCEWithLogitsLoss", DEV, Foreign(), n_iters=5)
    ref2, scale2, tor2 = _loss_bar("BCEWithLogitsLoss", [preds[i] for i in kept + [0]], [batches[i].y for i in kept + [0]],
                                   [sizes[i] for i in kept + [0]], sum(sizes))
    assert abs(loss2 - ref2) / scale2 <= max(2.0 * abs(tor2 - ref2) / scale2, FLOOR)
    with pytest.raises(TypeError):
        ev.test_ogb(loader, model, torch.nn.HuberLoss(), DEV, Foreign())

    # test(): regression with an L1 sum as the metric
    rb = [_Batch(bt.feat, bt.x, torch.randn(bt.feat.shape[0], n_tasks, generator=g)) for bt in batches]
    rl = _Loader(rb, sum(sizes) + 5)                                          # (division by len(loader.dataset), whatever was seen)
    loss, metric = ev.test(rl, model, torch.nn.L1Loss(), DEV, torch.nn.L1Loss(reduction="sum"))
    ref, scale, tor = _loss_bar("L1Loss", preds, [b.y for b in rb], sizes, sum(sizes) + 5)
    assert abs(loss - ref) / scale <= max(2.0 * abs(tor - ref) / scale, FLOOR)
    exact = [float((p.double() - b.y.double()).abs().sum()) for p, b in zip(preds, rb)]
    # (an fp32 sum per batch by definition: each within one fp32 ulp of the rounded float64 sum, see test_accumulator_metric_terms)
    assert abs(metric - sum(float(np.float32(e)) for e in exact) / (sum(sizes) + 5)) <= sum(float(np.spacing(np.float32(e))) for e in exact) / (sum(sizes) + 5)
    assert ev.test(rl, model, "MSELoss", DEV)[1] == 0.0
    # test(): classification, CrossEntropyLoss + multi_class_accuracy; ogbg-ppa through test_ogb
    cb = [_Batch(bt.feat, bt.x, torch.randint(0, n_tasks, (bt.feat.shape[0],), generator=g)) for bt in batches]
    cl = _Loader(cb, sum(sizes))
    loss, metric = ev.test(cl, model, torch.nn.CrossEntropyLoss(), DEV, ev.prediction_function("multi_class_accuracy"))
    ref, scale, tor = _loss_bar("CrossEntropyLoss", preds, [b.y for b in cb], sizes, sum(sizes))
    assert abs(loss - ref) / scale <= max(2.0 * abs(tor - ref) / scale, FLOOR)
    correct = sum(int((p.argmax(1) == b.y).sum()) for p, b in zip(preds, cb))
    assert metric == correct / sum(sizes)
    loss_p, acc_p = ev.test_ogb(cl, model, torch.nn.CrossEntropyLoss(), DEV, ev.Evaluator("ogbg-ppa"))
    kept_correct = sum(int((preds[i].argmax(1) == cb[i].y).sum()) for i in kept)
    assert acc_p == kept_correct / (sum(sizes) - 1)
