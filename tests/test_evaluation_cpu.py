"""CPU checks of the device-side evaluation (gsn_amd/evaluation.py, csrc/evaluate.hip): the referee tests/eval_ref.py against brute force and
against sklearn, the arithmetic of gsn_amd/csrc/evaluate_core.h run on the host by the test-only harness tests/evaluate_harness.cpp against
the referee, the argument checks of the entry points (decided on the host) and the name tables."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from eval_ref import KINDS, masked_loss_ref, normalised_error, rank_ref, u2_brute

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32P, F64P, I64P, U64P = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_int64, ctypes.c_uint64))
DENORM = np.float32(1e-45)           # the smallest positive denormal
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def lib():
    from gsn_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(REPO, "tests", "_build", "libevaluate_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "evaluate_harness.cpp")])
    return ctypes.CDLL(so)


def rank_cases(m, seed):
    """(name, scores fp32 [m], labels float [m] with NaN) -- heavy ties, +-0, denormals, tiny scales, NaN labels"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 2, size=m).astype(np.float64)
    yield "random", rng.standard_normal(m).astype(np.float32), lab
    yield "ties", rng.integers(0, 5, size=m).astype(np.float32), lab
    yield "all_equal", np.full(m, 0.25, dtype=np.float32), lab
    z = rng.choice(np.array([0.0, -0.0, DENORM, -DENORM, 2 * DENORM, 1e-30, -1e-30], dtype=np.float32), size=m)
    yield "zeros_denormals", z, lab
    yield "tiny", (rng.standard_normal(m) * 1e-30).astype(np.float32), lab
    nanlab = lab.copy()
    nanlab[rng.random(m) < 0.3] = np.nan
    yield "nan_labels", rng.integers(-3, 3, size=m).astype(np.float32), nanlab
    yield "one_class", rng.standard_normal(m).astype(np.float32), np.ones(m)
    yield "extremes", rng.choice(np.array([FMAX, -FMAX, 0.0, 1.0], dtype=np.float32), size=m), lab


@pytest.mark.parametrize("m", [1, 2, 3, 17, 257, 1025, 3000])
def test_referee_against_all_pairs(m):
    for name, s, l in rank_cases(m, m):
        r = rank_ref(s, l)
        assert r["u2"] == u2_brute(s, l), (name, m)
        assert r["n"] == int((~np.isnan(l)).sum()) and r["n_pos"] == int((l == 1).sum()), (name, m)


def test_referee_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    worst = [0.0, 0.0]
    for m in (2, 3, 64, 1025, 4097):
        for seed in range(6):
            for name, s, l in rank_cases(m, 100 * m + seed):
                keep = ~np.isnan(l)
                r = rank_ref(s, l)
                if r["auc"] is not None:
                    worst[0] = max(worst[0], abs(r["auc"] - metrics.roc_auc_score(l[keep], s[keep].astype(np.float64))))
                if r["ap"] is not None:
                    worst[1] = max(worst[1], abs(r["ap"] - metrics.average_precision_score(l[keep], s[keep].astype(np.float64))))
    print("referee against sklearn: worst difference auc %.3g ap %.3g" % tuple(worst))
    # a sequential float64 sum of M <= 4 097 terms of total <= 1: 4 097 * 2^-53 < 1e-12
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


def test_key_map_on_host(harness):
    vals = np.array([-FMAX, -1.0, -1e-30, -2 * DENORM, -DENORM, -0.0, 0.0, DENORM, 2 * DENORM, 1e-30, 1.0, FMAX], dtype=np.float32)
    keys = np.zeros(len(vals), dtype=np.uint64)
    for label in (0.0, 1.0):
        lab = np.full(len(vals), label, dtype=np.float32)
        harness.harness_keys(ctypes.c_int64(len(vals)), vals.ctypes.data_as(F32P), lab.ctypes.data_as(F32P), keys.ctypes.data_as(U64P))
        img = keys >> np.uint64(1)
        assert np.all((keys & np.uint64(1)) == np.uint64(label))
        assert img[5] == img[6]                                                   # -0.0 and +0.0 are tied
        order = np.concatenate([img[:5], img[6:]])
        assert np.all(order[1:] > order[:-1])                                     # strictly increasing through denormals and +-max
        assert np.all(keys < np.uint64(1 << 33))
    rng = np.random.default_rng(0)
    s = rng.standard_normal(5000).astype(np.float32) * np.float32(10.0) ** rng.integers(-38, 38, size=5000).astype(np.float32)
    lab = np.zeros(len(s), dtype=np.float32)
    keys = np.zeros(len(s), dtype=np.uint64)
    harness.harness_keys(ctypes.c_int64(len(s)), s.ctypes.data_as(F32P), lab.ctypes.data_as(F32P), keys.ctypes.data_as(U64P))
    o = np.argsort(s, kind="stable")
    assert np.all(np.diff(keys[o].astype(np.int64)) >= 0) and np.all((np.diff(keys[o].astype(np.int64)) == 0) == (np.diff(s[o]) == 0))
    # refused rows and unlabelled rows sort behind every valid key
    s = np.array([1.0, np.nan, np.inf, -np.inf, 1.0, 1.0], dtype=np.float32)
    lab = np.array([np.nan, 1.0, 0.0, 1.0, 2.0, -1.0], dtype=np.float32)
    keys = np.zeros(6, dtype=np.uint64)
    harness.harness_keys(ctypes.c_int64(6), s.ctypes.data_as(F32P), lab.ctypes.data_as(F32P), keys.ctypes.data_as(U64P))
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert keys.tolist() == [full, full - np.uint64(2), full - np.uint64(2), full - np.uint64(2), full - np.uint64(1), full - np.uint64(1)]


def _harness_rank(harness, s, l):
    s = np.ascontiguousarray(s, dtype=np.float32)
    l = np.ascontiguousarray(l, dtype=np.float32)
    oi, od = np.zeros(4, dtype=np.int64), np.zeros(1, dtype=np.float64)
    harness.harness_rank(ctypes.c_int64(len(s)), s.ctypes.data_as(F32P), l.ctypes.data_as(F32P), oi.ctypes.data_as(I64P), od.ctypes.data_as(F64P))
    return oi, od[0]


def boundary_tie_scores(m, rng):
    """increasing scores with tie runs over the sorted positions 1 000 .. 1 100 (a 1 024-chunk boundary) and 4 090 .. 4 100 (a 4 096-tile one)"""
    s = np.arange(m, dtype=np.float32)
    s[1000:1101] = s[1000]
    s[4090:4101] = s[4090]
    return s[rng.permutation(m)]


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8193, 12293])
def test_run_walk_on_host(harness, m):
    for name, s, l in rank_cases(m, 7 * m + 1):
        oi, ap = _harness_rank(harness, s, l)
        r = rank_ref(s, l)
        assert (int(oi[0]), int(oi[1]), int(oi[2]), int(oi[3])) == (r["n"], r["n_pos"], r["u2"], 0), (name, m)
        if r["ap"] is not None:
            assert abs(ap - r["ap"]) <= 1e-12, (name, m)
    if m >= 4101:
        rng = np.random.default_rng(m)
        s = boundary_tie_scores(m, rng)
        for share in (0.5, 0.02):
            l = (rng.random(m) < share).astype(np.float64)
            oi, ap = _harness_rank(harness, s, l)
            r = rank_ref(s, l)
            assert (int(oi[0]), int(oi[1]), int(oi[2])) == (r["n"], r["n_pos"], r["u2"]) and abs(ap - r["ap"]) <= 1e-12


def test_refused_rows_are_counted_out_on_host(harness):
    s = np.array([0.5, np.nan, 0.25, np.inf, 0.75, 0.1], dtype=np.float32)
    l = np.array([1.0, 0.0, 0.0, 1.0, 3.0, np.nan], dtype=np.float32)
    oi, _ = _harness_rank(harness, s, l)
    assert oi.tolist() == [2, 1, 2, 3]


def test_loss_formulas_on_host(harness):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(500) * 3, [0.0, -0.0, 100.0, -100.0, 100.0, -100.0, 1e-30, 88.0, -88.0, 700.0]]).astype(np.float32)
    y = np.concatenate([rng.integers(0, 2, size=500), [1, 0, 1, 1, 0, 0, 1, 0, 1, 1]]).astype(np.float32)
    n = len(x)
    loss, dloss = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float64)
    for kind in range(3):
        yy = y if kind == 0 else (y + rng.standard_normal(n)).astype(np.float32)
        harness.harness_loss(kind, ctypes.c_int64(n), x.ctypes.data_as(F32P), yy.ctypes.data_as(F32P), loss.ctypes.data_as(F32P), dloss.ctypes.data_as(F64P))
        assert np.all(np.isfinite(loss)) and np.all(np.isfinite(dloss))
        for i in range(n):      # element by element: the referee's mean over one labelled element is that element
            ref, scale, g, gs = masked_loss_ref(KINDS[kind], x[i:i + 1], yy[i:i + 1])
            assert abs(float(loss[i]) - ref) <= 2.0 ** -24 * scale + 1e-45, (kind, i, x[i], yy[i])
            assert abs(dloss[i] - g[0]) <= 1e-15 * max(gs[0], 1e-300) + (0 if gs[0] else 0), (kind, i)
        if kind:
            m = np.zeros(n, dtype=np.float32)
            harness.harness_metric(kind, ctypes.c_int64(n), x.ctypes.data_as(F32P), yy.ctypes.data_as(F32P), m.ctypes.data_as(F32P))
            assert np.array_equal(m, loss)
    # BCE stays finite where the naive form overflows
    big = np.array([100.0, -100.0], dtype=np.float32)
    one = np.array([0.0, 1.0], dtype=np.float32)
    harness.harness_loss(0, ctypes.c_int64(2), big.ctypes.data_as(F32P), one.ctypes.data_as(F32P), loss.ctypes.data_as(F32P), dloss.ctypes.data_as(F64P))
    assert loss[:2].tolist() == [100.0, 100.0]


@pytest.mark.parametrize("n_cls", [2, 37])
def test_cross_entropy_rows_on_host(harness, n_cls):
    rng = np.random.default_rng(n_cls)
    rows = 65
    x = (rng.standard_normal((rows, n_cls)) * 5).astype(np.float32)
    x[3] = x[3, 0]                       # a row of ties: arg-max is the first index
    x[4, :] = [100.0 if j % 2 else -100.0 for j in range(n_cls)]
    t = rng.integers(0, n_cls, size=rows).astype(np.int64)
    t[7], t[8] = -1, n_cls               # outside the classes: NaN loss, zero gradient row, no fault
    loss, drow, am = np.zeros(rows, dtype=np.float32), np.zeros((rows, n_cls), dtype=np.float64), np.zeros(rows, dtype=np.int64)
    harness.harness_ce(ctypes.c_int64(rows), ctypes.c_int64(n_cls), x.ctypes.data_as(F32P), t.ctypes.data_as(I64P), loss.ctypes.data_as(F32P),
                       drow.ctypes.data_as(F64P), am.ctypes.data_as(I64P))
    assert np.array_equal(am, x.argmax(axis=1)) and am[3] == 0
    assert math.isnan(loss[7]) and math.isnan(loss[8])
    for r in range(rows):
        if r in (7, 8):
            continue
        ref, scale, g, gs = masked_loss_ref("CrossEntropyLoss", x[r:r + 1], t[r:r + 1])
        assert abs(float(loss[r]) - ref) <= 2.0 ** -24 * scale
        assert normalised_error(drow[r], g[0], gs[0]) <= 1e-14


def test_entry_points_check_arguments_before_any_launch(lib):
    """Empty shapes launch nothing and succeed; null pointers with a non-empty shape, a short scratch, unknown kinds and shapes beyond the
    limits are refused -- all decided on the host, so this runs without a GPU."""
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    assert lib.gsn_masked_loss_fwd_hip(0, 0, 3, None, None, None, None, None, 0, None) == 0
    assert lib.gsn_masked_loss_fwd_hip(0, 5, 0, None, None, None, None, None, 0, None) == 0
    # CrossEntropyLoss rows without a class column have no target class and no maximum to read: refused whatever the other pointers are
    # (empty shapes WITH somewhere to write the NaN launch a kernel: test_evaluation_gpu.py::test_empty_shapes)
    assert lib.gsn_masked_loss_fwd_hip(3, 5, 0, None, None, None, None, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(3, 5, 0, None, p, p, p, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(3, 5, 0, p, p, p, p, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(3, 0, 5, None, None, None, None, None, 0, None) == 0
    assert lib.gsn_masked_loss_fwd_hip(0, 5, 2, None, None, None, None, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(0, 5, 2, p, p, None, None, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(9, 5, 2, p, p, p, p, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(0, -1, 2, p, p, p, p, None, 0, None) == -1
    assert lib.gsn_masked_loss_fwd_hip(0, 70001, 1, p, p, p, p, None, 0, None) == -1       # the two-launch path needs scratch
    assert lib.gsn_masked_loss_fwd_hip(0, 70001, 1, p, p, p, p, p, 8, None) == -4          # GSN_E_NOSPACE
    assert lib.gsn_masked_loss_bwd_hip(0, 0, 3, None, None, None, None, None, None) == 0
    assert lib.gsn_masked_loss_bwd_hip(0, 5, 2, None, None, None, None, None, None) == -1
    assert lib.gsn_masked_loss_bwd_hip(3, 5, 0, p, p, p, p, p, None) == -1
    assert lib.gsn_masked_loss_bwd_hip(0, 5, 2, p, p, None, None, None, None) == -1
    f = lib.gsn_masked_loss_scratch_bytes
    assert f(0, 65536, 1) == 0 and f(0, 512, 128) == 0 and f(0, 0, 5) == 0 and f(7, 70001, 1) == 0
    assert f(0, 65537, 1) >= 32 * 65 and f(3, 70001, 2) >= 32 * 69 and f(0, 65537, 1) % 256 == 0
    assert lib.gsn_eval_accumulate_scratch_bytes(1, 70001, 3) == f(1, 70001, 3)
    acc = lib.gsn_eval_accumulate_hip
    assert acc(0, 0, 0, 3, 3, None, None, 0, None, None, None, None, 0, None, None, 0, None) == 0
    assert acc(0, 0, 5, 2, 2, None, None, 5, None, None, None, None, 10, None, None, 0, None) == -1
    assert acc(3, 0, 5, 0, 1, None, p, 5, p, p, None, None, 10, None, None, 0, None) == -1         # CrossEntropyLoss rows of 0 classes
    assert acc(0, 0, 5, 2, 2, p, p, 5, None, None, None, None, 10, None, None, 0, None) == -1      # no accumulators
    assert acc(0, 7, 5, 2, 2, p, p, 5, p, p, None, None, 10, None, None, 0, None) == -1            # unknown metric
    assert acc(0, 3, 5, 2, 2, p, p, 5, p, p, None, None, 10, None, None, 0, None) == -1            # accuracy needs integer targets
    assert acc(3, 1, 5, 2, 1, p, p, 5, p, p, None, None, 10, None, None, 0, None) == -1            # an L1 sum of class indices
    assert acc(0, 0, 5, 2, 1, p, p, 5, p, p, None, None, 10, None, None, 0, None) == -1            # target width
    assert acc(0, 0, 5, 2, 2, p, p, 5, p, p, None, None, -1, None, None, 0, None) == -1
    rk = lib.gsn_rank_metrics_hip
    assert rk(5, 0, None, None, None, None, None, None, 0, None) == 0
    assert rk(5, 2, None, None, None, None, None, None, 0, None) == -1
    assert rk(5, 2, p, p, p, p, p, None, 0, None) == -1
    assert rk(5, 2, p, p, p, p, p, p, 8, None) == -4
    assert rk(1 << 31, 1, p, p, p, p, p, p, 1 << 40, None) == -2                                   # GSN_E_UNSUPPORTED
    assert rk(5, 65536, p, p, p, p, p, p, 1 << 40, None) == -2
    assert rk(-1, 2, p, p, p, p, p, p, 8, None) == -1
    g = lib.gsn_rank_metrics_scratch_bytes
    assert g(0, 3) == 0 and g(5, 0) == 0 and g(5, 2) >= 80 and g(4097, 3) >= 8 * 4097 * 3 and g(4097, 3) % 256 == 0


def test_name_tables_and_evaluator_table():
    import torch
    from gsn_amd import evaluation as ev
    for name in KINDS:
        fn = ev.loss_function(name)
        assert isinstance(fn, ev.MaskedLoss) and fn.kind == name and ev._loss_name(fn) == name
    with pytest.raises(NotImplementedError):
        ev.loss_function("HuberLoss")
    assert ev.prediction_function("None") is None
    for name in ("multi_class_accuracy", "MSELoss", "L1Loss"):
        assert ev.prediction_function(name).name == name
    with pytest.raises(NotImplementedError):
        ev.prediction_function("f1")
    # torch's own loss objects are named by class, with default arguments only
    assert ev._loss_name(torch.nn.BCEWithLogitsLoss()) == "BCEWithLogitsLoss" and ev._loss_name(torch.nn.CrossEntropyLoss()) == "CrossEntropyLoss"
    assert ev._loss_name(torch.nn.L1Loss()) == "L1Loss" and ev._loss_name(torch.nn.MSELoss()) == "MSELoss"
    for bad in (torch.nn.MSELoss(reduction="sum"), torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(1)), torch.nn.CrossEntropyLoss(label_smoothing=0.1),
                torch.nn.HuberLoss(), lambda a, b: a):
        with pytest.raises(TypeError):
            ev._loss_name(bad)
    assert ev._metric_name(torch.nn.L1Loss(reduction="sum")) == "L1Loss" and ev._metric_name(None) is None

    def multi_class_accuracy(y_hat, y):
        return None
    assert ev._metric_name(multi_class_accuracy) == "multi_class_accuracy"
    with pytest.raises(TypeError):
        ev._metric_name(torch.nn.L1Loss())
    assert (ev.Evaluator("ogbg-molhiv").eval_metric, ev.Evaluator("ogbg-molpcba").eval_metric, ev.Evaluator("ogbg-ppa").eval_metric) == ("rocauc", "ap", "acc")
    e = ev.Evaluator("my-set", eval_metric="ap")
    assert e.name == "my-set" and e.eval_metric == "ap"
    with pytest.raises(ValueError):
        ev.Evaluator("my-set")
    with pytest.raises(ValueError):
        ev.Evaluator("ogbg-molhiv", eval_metric="f1")


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gsn_amd import evaluation as ev
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.masked_loss("BCEWithLogitsLoss", torch.zeros(4, 1), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.Evaluator("ogbg-molhiv").eval({"y_true": np.zeros((4, 1)), "y_pred": np.zeros((4, 1))})
