"""The row-bounded BatchNorm entries and the counted masked loss on the GPU, called through the ABI: a padded batch's real rows
are the prefix [0, v) of the m_rows rows a stage runs over, v = clamp(row_ptr ? row_ptr[clamp(*n_valid, 0, n_slots)] : *n_valid, 0, m_rows)
read on the device.  Reference: the float64 referee tests/bn_ref.py applied to the first v rows; bars: those of tests/test_bn_kernels_gpu.py
for the same quantities (gH 16, column sums 8, bias gradient 16 / 8, in units of 2^-24 of bn_ref's magnitudes; the finalize vectors 2 fp32 ulp
of the float64 bookkeeping) -- see _vector_bars for what the statistics' own error adds under the tail subtraction.

What the rows behind v hold is chosen so that ONE leaked row is far outside every bar: pre-BN rows of another scale (x 64, offset 1e3),
NaN gradients, NaN / infinite predictions and out-of-range classes."""
import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu
E = R.EPS
EPS_BN = 1e-5
TINY = 1e-300
# m_rows: 9001 is above the finalize kernel's grid cap (64 workgroups x 64 rows of the half range): its waves walk several strides and 64
# workgroups per column group meet at the ticket
SHAPES = [(m, c) for m in (2, 3, 64, 65, 257, 4099) for c in (1, 3, 64, 65, 300)] + [(9001, 3), (9001, 65)]


def _lib():
    from gsn_amd import _abi
    return _abi, _abi.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _ff(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _seed(*k):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31))


def _values_of_v(m):
    return sorted({0, 1, 2, m // 2, m // 2 + 1, m - 1, m} & set(range(m + 1)))


def _bounds(v, m, seed):
    """the same v given four ways: (n_valid, row_ptr or None) directly, through a row_ptr, and with *n_valid clamped from below / above"""
    rng = np.random.default_rng(seed)
    n_slots = 5
    out = [(v, None)]
    k = int(rng.integers(0, n_slots + 1))
    ptr = np.sort(rng.integers(0, m + 1, n_slots + 1)).astype(np.int64)
    ptr[k] = v
    out.append((k, ptr))
    if v == 0:
        out.append((-5, None))
        low = ptr.copy(); low[0] = 0; low[1:] = m
        out.append((-5, low))
    if v == m:
        out.append((m + 7, None))
    high = ptr.copy(); high[n_slots] = v
    out.append((n_slots + 7, high))
    return out


def _bound_args(n_valid, ptr):
    nv = torch.tensor([n_valid], dtype=torch.int64, device="cuda")
    rp = _dev(ptr)
    return nv, rp, (nv.data_ptr(), None if rp is None else rp.data_ptr(), 0 if rp is None else rp.numel() - 1)


# ----------------------------------------------------------------------------------------------------------------------
# forward: gsn_bn_finalize_bounded_hip
# ----------------------------------------------------------------------------------------------------------------------
def _finalize_bounded(m, c, stats, h, bound, gamma, beta, running, momentum, nbt):
    _abi, L = _lib()
    vec = _ff((4, c))
    p0 = vec.data_ptr()
    nbytes = int(L.gsn_bn_finalize_bounded_scratch_bytes(c))
    scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
    nv, rp, (a, b, n) = _bound_args(*bound)
    rc = L.gsn_bn_finalize_bounded_hip(c, m, EPS_BN, float(momentum), stats.data_ptr(), h.data_ptr(), a, b, n, scratch.data_ptr(), gamma.data_ptr(),
                                       beta.data_ptr(), running[0].data_ptr(), running[1].data_ptr(), p0, p0 + 4 * c, p0 + 8 * c, p0 + 12 * c,
                                       nbt.data_ptr(), _abi.current_stream())
    _abi.check(rc, "gsn_bn_finalize_bounded_hip")
    return _np(vec)


def _finalize_count(m, c, stats, gamma, beta, running, momentum, nbt):
    _abi, L = _lib()
    vec = _ff((4, c))
    p0 = vec.data_ptr()
    rc = L.gsn_bn_finalize_count_hip(c, m, EPS_BN, float(momentum), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), running[0].data_ptr(),
                                     running[1].data_ptr(), p0, p0 + 4 * c, p0 + 8 * c, p0 + 12 * c, nbt.data_ptr(), _abi.current_stream())
    _abi.check(rc, "gsn_bn_finalize_count_hip")
    return _np(vec)


def _vector_bars(h64, v, m, ref, gamma, momentum):
    """Absolute bars of (mean, invstd, scale, running_mean, running_var) around the float64 bookkeeping of the first v rows.

    The bookkeeping itself is held to 2 fp32 ulp (test_bn_kernels_gpu.py: test_finalize_entries_against_float64_bookkeeping).  The SUMS it
    starts from carry the statistics' bar of that file, 1 unit = M 2^-53 (sum |x|, sum x^2) -- the worst case of adding M fp64 terms -- with M
    and the magnitudes those of the rows that were actually added or cancelled: the first v rows when v <= m - v (summed directly), ALL m rows
    otherwise (the given sums over m rows minus the kernel's sums over the tail).  Propagated to first order:
        d mean = u1 / v,   d var = u2 / v + 2 |mean| u1 / v,   d invstd = invstd^3 d var / 2,   d scale = |gamma| d invstd,
        d running_mean = momentum d mean,   d running_var = momentum d var v / (v - 1)."""
    rows = h64[:v] if v <= m - v else h64
    M = rows.shape[0]
    u1 = M * 2.0 ** -53 * np.abs(rows).sum(0)
    u2 = M * 2.0 ** -53 * (rows * rows).sum(0)
    d_mean = u1 / v
    d_var = u2 / v + 2.0 * np.abs(ref["mean"]) * u1 / v
    d_inv = 0.5 * ref["invstd"] ** 3 * d_var
    g = np.abs(gamma.astype(np.float64))
    return {"mean": d_mean, "invstd": d_inv, "scale": g * d_inv, "rm": momentum * d_mean, "rv": momentum * d_var * (v / (v - 1.0 if v > 1 else 1.0))}


@pytest.mark.parametrize("m,c", SHAPES)
def test_finalize_bounded_takes_the_statistics_of_the_first_v_rows(m, c):
    rng = np.random.default_rng(_seed(m, c, 71))
    base = (rng.normal(0.0, 2.0, c) + rng.normal(0.0, 1.0, (m, c)) / rng.uniform(0.2, 5.0, c)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    beta = rng.normal(0.0, 0.5, c).astype(np.float32)
    g_d, b_d = _dev(gamma), _dev(beta)
    momentum = 0.1
    worst = 0.0
    for v in _values_of_v(m):
        h = base.copy()
        h[v:] = h[v:] * 64.0 + 1e3                  # pad rows: finite, another scale
        h64 = h.astype(np.float64)
        stats_all = np.stack([h64.sum(0), (h64 * h64).sum(0)])          # what the product kernels hand over: the sums over ALL m rows
        h_d, st_d = _dev(h), _dev(stats_all)
        for bi, bound in enumerate(_bounds(v, m, _seed(m, c, v))):
            run = [torch.full((c,), 0.25, device="cuda"), torch.full((c,), 1.5, device="cuda")]
            nbt = torch.tensor(7, dtype=torch.int64, device="cuda")
            vec = _finalize_bounded(m, c, st_d, h_d, bound, g_d, b_d, run, momentum, nbt)
            tag = "%d x %d v %d bound %d" % (m, c, v, bi)
            assert int(nbt) == 8, tag
            assert np.isfinite(vec).all(), tag
            if v == 0:
                assert np.array_equal(vec, np.stack([np.zeros(c), np.ones(c), np.ones(c), np.zeros(c)]).astype(np.float32)), tag
                assert np.array_equal(_np(run[0]).view(np.uint32), np.full(c, 0.25, np.float32).view(np.uint32)), tag
                assert np.array_equal(_np(run[1]).view(np.uint32), np.full(c, 1.5, np.float32).view(np.uint32)), tag
                continue
            real = np.stack([h64[:v].sum(0), (h64[:v] * h64[:v]).sum(0)])
            ref = R.bn_vectors(real, v, EPS_BN, gamma, beta)
            if v == 1:                                  # one real row: variance 0 exactly, invstd 1 / sqrt(eps), everything finite
                assert np.array_equal(vec[1], np.full(c, np.float32(1.0 / np.sqrt(np.float64(EPS_BN))))), tag
                assert np.array_equal(vec[0], h[0]), tag
            bars = _vector_bars(h64, v, m, ref, gamma, momentum)
            rm, rv = R.running_update(np.full(c, 0.25), np.full(c, 1.5), ref["mean"], ref["var"], v, momentum)
            for got, want, bar in ((vec[0], ref["mean"], bars["mean"]), (vec[1], ref["invstd"], bars["invstd"]), (vec[2], ref["scale"], bars["scale"]),
                                   (_np(run[0]), rm, bars["rm"]), (_np(run[1]), rv, bars["rv"])):
                err = np.abs(got.astype(np.float64) - want)
                u = (err / (2.0 * R.ulp32(want) + bar)).max()
                worst = max(worst, u)
                assert u <= 1.0, (tag, u)
            assert np.array_equal(vec[3], beta), tag
            if v == m:          # the whole capacity is real: the bits of gsn_bn_finalize_count_hip on the same sums, running statistics and counter too
                run2 = [torch.full((c,), 0.25, device="cuda"), torch.full((c,), 1.5, device="cuda")]
                nbt2 = torch.tensor(7, dtype=torch.int64, device="cuda")
                vec2 = _finalize_count(m, c, st_d, g_d, b_d, run2, momentum, nbt2)
                assert np.array_equal(vec.view(np.uint32), vec2.view(np.uint32)), tag
                assert torch.equal(run[0], run2[0]) and torch.equal(run[1], run2[1]) and int(nbt2) == int(nbt), tag
    print("bn-bounded finalize %d x %d: worst %.3f of 1 (2 ulp + the sums' bar)" % (m, c, worst))


# ----------------------------------------------------------------------------------------------------------------------
# backward: gsn_bn_act_bwd_from_h_bounded_hip
# ----------------------------------------------------------------------------------------------------------------------
def _bwd(case, gy, act, train_bn, bound=None):
    _abi, L = _lib()
    m, c = case["h"].shape
    gy_d, h = _dev(gy), _dev(case["h"])
    mean, invstd, coef, shift = (_dev(case[k]) for k in ("mean", "invstd", "coef", "beta"))
    sums = torch.zeros(2, c, dtype=torch.float64, device="cuda")
    gbias = torch.zeros(c, dtype=torch.float64, device="cuda")
    gh = _ff((m, c))
    head = (m, c, gy_d.data_ptr(), h.data_ptr(), mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), shift.data_ptr(), train_bn, act, sums.data_ptr(),
            gh.data_ptr(), gbias.data_ptr())
    if bound is None:
        _abi.check(L.gsn_bn_act_bwd_from_h_hip(*head, _abi.current_stream()), "gsn_bn_act_bwd_from_h_hip")
    else:
        nv, rp, ptrs = _bound_args(*bound)
        _abi.check(L.gsn_bn_act_bwd_from_h_bounded_hip(*head, *ptrs, _abi.current_stream()), "gsn_bn_act_bwd_from_h_bounded_hip")
    return gh, _np(sums), _np(gbias)


@pytest.mark.parametrize("m,c", SHAPES)
def test_bwd_bounded_sums_the_first_v_rows_and_zeroes_the_rest(m, c):
    case = R.make_case(m, c, _seed(m, c, 72))
    misses, worst = [], [0.0, 0.0, 0.0]
    for vi, v in enumerate(_values_of_v(m)):
        gy = case["gy"].copy()
        gy[v:] = np.nan                            # never read: a NaN that entered a sum or a row would stay
        act = vi % 4
        for train_bn in (1, 2):
            # the float64 adjoint of the first v rows, once; per call below gH is formed from the sums THAT call's reduce pass wrote, as
            # bn_ref.adjoint(sums=...) does (the apply pass by itself), the sums are held to the float64 ones
            a0 = R.adjoint(gy[:v], case["h"][:v], case["mean"], case["invstd"], case["coef"], case["beta"], act, train_bn) if v else None
            for bi, bound in enumerate(_bounds(v, m, _seed(m, c, v, 3))):
                tag = "%d x %d v %d act %d train_bn %d bound %d" % (m, c, v, act, train_bn, bi)
                gh_t, sums, gbias = _bwd(case, gy, act, train_bn, bound)
                gh = _np(gh_t)
                assert not np.any(gh[v:].view(np.uint32)), tag + ": rows behind v are not +0"
                assert np.isfinite(gh).all() and np.isfinite(sums).all() and np.isfinite(gbias).all(), tag
                if v == 0:
                    assert not sums.any() and not gbias.any(), tag
                    continue
                a = dict(a0)
                if train_bn == 1:
                    m1, m2 = sums[0] / v, sums[1] / v
                    a["gh"] = a0["gh_coef"] * (a0["gz"] - m1 - a0["xhat"] * m2)
                    a["bound"] = np.abs(a0["gh_coef"]) * (a0["gz_mag"] + np.abs(m1) + np.abs(a0["xhat"] * m2))
                    a["g_bias"], a["g_bias_abs"] = a["gh"].sum(0), a["bound"].sum(0)
                u_gh = (np.abs(gh[:v].astype(np.float64) - a["gh"]) / (E * a["bound"])).max()
                u_s = max((np.abs(sums[0] - a["s1"]) / (E * a["s1_abs"] + TINY)).max(), (np.abs(sums[1] - a["s2"]) / (E * a["s2_abs"] + TINY)).max())
                if train_bn == 1:
                    u_b = (np.abs(gbias - a["g_bias"]) / (E * a["g_bias_abs"])).max() / 16.0
                else:
                    u_b = (np.abs(gbias - a["g_bias"]) / (E * np.abs(a["gh"]).sum(0) + TINY)).max() / 8.0
                worst = [max(worst[0], u_gh), max(worst[1], u_s), max(worst[2], u_b)]
                if u_gh > 16.0 or u_s > 8.0 or u_b > 1.0:
                    misses.append("%s: gH %.2f of 16, sums %.2f of 8, bias gradient %.2f of 1" % (tag, u_gh, u_s, u_b))
                if v == m and m <= 64 and bi == 0:        # one workgroup per column group: no atomic reordering -> the unbounded entry's bits
                    gh0, sums0, gbias0 = _bwd(case, case["gy"], act, train_bn)
                    assert torch.equal(gh_t.view(torch.int32), gh0.view(torch.int32)), tag
                    assert np.array_equal(sums, sums0) and np.array_equal(gbias, gbias0), tag
    print("bn-bounded adjoint %d x %d: gH %.3f of 16, sums %.3f of 8, bias gradient %.3f of 1" % (m, c, worst[0], worst[1], worst[2]))
    assert not misses, misses


# ----------------------------------------------------------------------------------------------------------------------
# counted masked loss
# ----------------------------------------------------------------------------------------------------------------------
KINDS = {"BCEWithLogitsLoss": 0, "L1Loss": 1, "MSELoss": 2, "CrossEntropyLoss": 3}


def _loss(kind, rows, cols, y_hat, y, n_valid=None):
    """(loss, count, grad) of one forward + backward through the plain entries (rows = the row count they see) or the counted ones"""
    _abi, L = _lib()
    k = KINDS[kind]
    loss = _ff(()); count = _ff((), torch.int64)
    grad = _ff((max(rows, 1), cols))[:rows]
    nb = int(L.gsn_masked_loss_scratch_bytes(k, rows, cols))
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda") if nb else None
    one = torch.tensor(1.0, device="cuda")
    wsp = None if ws is None else ws.data_ptr()
    if n_valid is None:
        _abi.check(L.gsn_masked_loss_fwd_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), loss.data_ptr(), count.data_ptr(), wsp, nb, _abi.current_stream()), "fwd")
        _abi.check(L.gsn_masked_loss_bwd_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), one.data_ptr(), count.data_ptr(), grad.data_ptr(),
                                             _abi.current_stream()), "bwd")
    else:
        _abi.check(L.gsn_masked_loss_fwd_counted_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), n_valid.data_ptr(), loss.data_ptr(), count.data_ptr(),
                                                     wsp, nb, _abi.current_stream()), "fwd counted")
        _abi.check(L.gsn_masked_loss_bwd_counted_hip(k, rows, cols, y_hat.data_ptr(), y.data_ptr(), n_valid.data_ptr(), one.data_ptr(), count.data_ptr(),
                                                     grad.data_ptr(), _abi.current_stream()), "bwd counted")
    return loss, count, grad


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("rows,cols", [(37, 3), (70001, 1), (14000, 5)])       # one launch / two launches (rows x cols > 65 536)
def test_counted_loss_is_the_plain_loss_of_the_first_v_rows(kind, rows, cols):
    rng = np.random.default_rng(_seed(rows, cols, KINDS[kind]))
    ce = kind == "CrossEntropyLoss"
    cols = max(cols, 2) if ce else cols
    yh = rng.normal(0.0, 2.0, (rows, cols)).astype(np.float32)
    if ce:
        y = rng.integers(0, cols, rows).astype(np.int64)
    else:
        y = (rng.integers(0, 2, (rows, cols)) if kind == "BCEWithLogitsLoss" else rng.normal(0.0, 1.0, (rows, cols))).astype(np.float32)
        y[rng.random((rows, cols)) < 0.2] = np.nan
    for v, nv in ((0, 0), (0, -5), (1, 1), (rows // 2, rows // 2), (rows - 1, rows - 1), (rows, rows), (rows, rows + 7)):
        yh_v, y_v = yh.copy(), y.copy()
        yh_v[v::3] = np.nan; yh_v[v + 1::3] = np.inf; yh_v[v + 2::3] = -np.inf       # rows behind v: never read
        if ce:
            y_v[v::2] = cols + 99; y_v[v + 1::2] = -3
        else:
            y_v[v:] = 1.0                                                          # labelled, were they looked at
        yh_d, y_d = _dev(yh_v), _dev(y_v)
        n_valid = torch.tensor([nv], dtype=torch.int64, device="cuda")
        loss, count, grad = _loss(kind, rows, cols, yh_d, y_d, n_valid)
        loss0, count0, grad0 = _loss(kind, v, cols, yh_d, y_d)
        tag = "%s %d x %d n_valid %d" % (kind, rows, cols, nv)
        assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32)), tag
        assert torch.equal(count, count0), tag
        assert torch.equal(grad[:v].view(torch.int32), grad0.view(torch.int32)), tag
        assert not bool(grad[v:].view(torch.int32).any()), tag + ": gradient rows behind v are not +0"


# ----------------------------------------------------------------------------------------------------------------------
# the bound object (the checks behind a device-resident n_valid: tests/test_bn_bounded_cpu.py covers n_valid itself)
# ----------------------------------------------------------------------------------------------------------------------
def test_row_bound_validates_row_ptr_and_host_rows():
    from gsn_amd._bound import RowBound
    nv = torch.zeros(1, dtype=torch.int64, device="cuda")
    ptr = torch.arange(6, dtype=torch.int64, device="cuda")
    b = RowBound(nv, ptr, 4)
    assert (b.n_slots, b.host_rows, b.used) == (5, 4, 0) and b.pointers() == (nv.data_ptr(), ptr.data_ptr(), 5)
    assert RowBound(nv).pointers() == (nv.data_ptr(), None, 0)
    for bad in (ptr.to(torch.int32), ptr.view(2, 3), torch.arange(12, dtype=torch.int64, device="cuda")[::2], ptr[:0], [0, 1, 2]):
        with pytest.raises(TypeError, match="row_ptr is a contiguous 1-D int64 tensor"):
            RowBound(nv, bad)
    with pytest.raises(TypeError, match="row_ptr lives on"):
        RowBound(nv, ptr.cpu())
    for bad in (-1, 2.0, True):
        with pytest.raises(TypeError, match="host_rows"):
            RowBound(nv, ptr, bad)
