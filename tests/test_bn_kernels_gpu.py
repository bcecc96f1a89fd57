"""Every pass of the BatchNorm + activation stage kernels (csrc/backward.hip, the tail of csrc/encode.hip) by direct ABI calls against the
float64 reference of tests/bn_ref.py: forward (bn_act_kernel below 64 rows, bn_act_cols_kernel from 64, the row pass of
bn_finalize_act_kernel, bn_act_planes_kernel), the adjoint passes (reduce + apply from y and from h, bn_act_bwd_planes_kernel), the fp16x3
row scratch both plane kernels write (decoded: scales, planes, padding), the [2][C] statistics of every producer, the bookkeeping of the three
finalize entries, and where the raw-moment variance stops agreeing with a two-pass evaluation.

Output buffers are pre-filled with NaN bytes: an element a kernel leaves out is seen.  Row counts: 1, 2, 3, 63, 64, 65, 257, 4099 and one above each
grid cap (16 401: bn_finalize_act's 1024 workgroups x 16 rows; 65 601: bgrid's 1024 x 64 rows and the plane kernels' 2048 x 32; 131 201:
gsn_bn_act_hip's 2048 x 64) -- from there a wave walks several strides of its row loop, unrolled body and tail.  Bars are in units of
2^-24 (R.EPS) of the magnitudes bn_ref states; each test prints its worst figure ("bn-bars ...") before it asserts."""
import itertools

import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

E = R.EPS
ROWS = (1, 2, 3, 63, 64, 65, 257, 4099)
COL_SHAPES = [(m, 3) for m in ROWS] + [(m, c) for m in (65, 257) for c in (1, 63, 64, 65, 130)]
PLANE_SHAPES = [(m, 4 if i % 2 == 0 else 8) for i, m in enumerate(ROWS)] + [(m, c) for m in (65, 257) for c in (28, 32, 36, 300, 640)]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_figures():
    yield
    for k in sorted(WORST):
        print("bn-bars worst %-28s %8.3f" % (k, WORST[k]))


def _note(key, value):
    value = float(value)
    WORST[key] = max(WORST.get(key, 0.0), value)
    return value


def _lib():
    from gsn_amd import _abi
    return _abi, _abi.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _np(t):
    return t.detach().cpu().numpy()


def _seed(*k):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31))


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def _forward_units(y, h, mean, scale, shift, act):
    """worst |y - ref| in units of 2^-24 (|(h - mean) scale| + |shift| + |ref|); the bar is 8"""
    assert not np.isnan(y).any(), "an element was left unwritten (or came out NaN)"
    ref, mag = R.forward(h, mean, scale, shift, act)
    return (np.abs(y.astype(np.float64) - ref) / (E * mag)).max()


def _bn_act(case, act, inplace, has=(True, True, True)):
    _abi, L = _lib()
    m, c = case["h"].shape
    h = _dev(case["h"])
    vec = [_dev(case[k]) if on else None for k, on in zip(("mean", "coef", "beta"), has)]
    out = h if inplace else _nan((m, c))
    _abi.check(L.gsn_bn_act_hip(m, c, h.data_ptr(), _p(vec[0]), _p(vec[1]), _p(vec[2]), act, out.data_ptr(), _abi.current_stream()), "gsn_bn_act_hip")
    args = [case[k] if on else None for k, on in zip(("mean", "coef", "beta"), has)]
    return _forward_units(_np(out), case["h"], args[0], args[1], args[2], act)


@pytest.mark.parametrize("m,c", COL_SHAPES + [(131201, 4)])
def test_bn_act_forward(m, c):
    """gsn_bn_act_hip: every activation out of place, relu in place, and each of mean / scale / shift null or given (elu, alternately in place
    and out of place) -- bn_act_kernel below 64 rows, bn_act_cols_kernel from 64 (131 201 rows: 2048 workgroups x 4 waves walk 17 strides)."""
    worst = 0.0
    case = R.make_case(m, c, _seed(m, c, 1))
    for act in range(4):
        worst = max(worst, _bn_act(case, act, False))
    worst = max(worst, _bn_act(case, 1, True))
    for i, has in enumerate(itertools.product((False, True), repeat=3)):
        if all(has):
            continue
        sub = R.make_case(m, c, _seed(m, c, 2 + i), *has)
        worst = max(worst, _bn_act(sub, 2, i % 2 == 1, has))
    print("bn-bars forward bn_act %d x %d: %.3f of 8" % (m, c, _note("forward (bar 8)", worst)))
    assert worst <= 8.0


# ----------------------------------------------------------------------------------------------------------------------
# adjoint, column kernels
# ----------------------------------------------------------------------------------------------------------------------
TINY = 1e-300         # (relu with every z of a column negative: sum and magnitude are both exactly 0 -- 0 / TINY = 0 units)


def _bar(misses, tag, name, stated, bar, consistent=None):
    """One figure against its bar.  ``stated``: the figure in the units the bar was set in.  The bars of the sums and of the bias gradient
    (8 units of sum_r |term|) sit close to the worst case of the roundings of ONE term (_check_adjoint); for those ``consistent`` is the same
    error against a magnitude with room for that, in units of ITS bar: asserted at once -- a miss is a defect of the kernel -- while a miss
    of the stated bar goes to ``misses``, asserted when the rest of the test has been checked, so that it hides nothing else."""
    _note("%s (bar %g)" % (name, bar), stated)
    if consistent is None:
        assert stated <= bar, (tag, name, stated)
    else:
        _note("%s, with the error the bar leaves out (bar 1)" % name, consistent)
        assert consistent <= 1.0, (tag, name, consistent)
        if stated > bar:
            misses.append("%s: %s %.2f of %g" % (tag, name, stated, bar))
    return stated


def _check_sums(sums, a, misses, tag):
    e1, e2 = np.abs(sums[0] - a["s1"]), np.abs(sums[1] - a["s2"])
    stated = max((e1 / (E * a["s1_abs"] + TINY)).max(), (e2 / (E * a["s2_abs"] + TINY)).max())
    consistent = max((e1 / (8.0 * E * a["s1_mag"])).max(), (e2 / (8.0 * E * a["s2_mag"] + TINY)).max())
    return _bar(misses, tag, "sums", stated, 8.0, consistent)


def _check_adjoint(a, gh, sums, gbias, train_bn, tag, misses, batch_stats=False):
    """gH element-wise: |gH - ref| in units of 2^-24 bound, bar 16.  The two sums and the bias gradient: units of 2^-24 sum_r |term|, bar 8.
    train_bn 1: the bias gradient's true value is zero when mean / invstd ARE the batch statistics of h (``batch_stats``: |grad_bias| within
    16 units of sum_r bound); with vectors drawn independently of h it is -coef m2 sum_r xhat, and the kernel's sum is held to the same
    16 units around that.

    ``a``: R.adjoint with ``sums`` = the sums the kernel's reduce pass wrote, so that gH is the apply pass by itself; the sums are held to
    float64 on their own bar.

    The bar of the sums and of the bias gradient, 8 units of sum_r |term|: a term gZ xhat = gY act' xhat carries up to about nine roundings
    (e^x at one ulp, 1 + u, its square, the quotient, the products, the difference h - mean), and a column of one row has nothing to
    average them over; measured, the worst column stays under half the bar.  What brings these sums under it at all is that the kernels form
    act' with a RELATIVE error (backward.hip: act_grad_from_y, act_grad_from_h; test_saturated_units_...).  Beside the stated bar the same
    error is held, at once, to 8 units of sum_r |gY| max(1, |act'|) (times |xhat|; the bias gradient: of sum_r bound) -- _bar."""
    assert not np.isnan(gh).any(), "an element of grad_h was left unwritten (or came out NaN)"
    err = np.abs(gh.astype(np.float64) - a["gh"])
    figs = [0.0, 0.0, 0.0]
    figs[0] = _bar(misses, tag, "adjoint gH, train_bn %s" % ("1" if train_bn == 1 else "0 and 2"), (err / (E * a["bound"])).max(), 16.0)
    if train_bn:
        figs[1] = _check_sums(sums, a, misses, tag)
    if train_bn == 1 and batch_stats:
        figs[2] = _bar(misses, tag, "bias gradient, batch statistics", (np.abs(gbias) / (E * a["g_bias_abs"])).max(), 16.0)
    elif train_bn == 1:
        figs[2] = _bar(misses, tag, "bias gradient, train_bn 1, drawn vectors", (np.abs(gbias - a["g_bias"]) / (E * a["g_bias_abs"])).max(), 16.0)
    else:
        eb = np.abs(gbias - a["g_bias"])
        figs[2] = _bar(misses, tag, "bias gradient", (eb / (E * np.abs(a["gh"]).sum(0) + TINY)).max(), 8.0, (eb / (8.0 * E * a["g_bias_abs"])).max())
    print("bn-bars adjoint %s: gH %.3f of 16, sums %.3f of 8, bias gradient %.3f of %d" % (tag, figs[0], figs[1], figs[2], 16 if train_bn == 1 else 8))


def _batch_case(m, c, seed):
    """a case whose mean / invstd are the batch statistics of its own rows (fp32 roundings of the float64 bookkeeping), as a train-mode stage
    hands them to its adjoint: the setting in which the bias gradient under train_bn 1 is zero"""
    h, gamma, beta, stats = _stage_rows(m, c, seed)
    v = R.bn_vectors(stats, m, EPS_BN, gamma, beta)
    mean, invstd = v["mean"].astype(np.float32), v["invstd"].astype(np.float32)
    coef = (gamma * invstd).astype(np.float32)
    z = R.pre_activation(h, mean, coef, beta)
    assert np.abs(z).min() >= R.Z_MIN_ASSERTED, np.abs(z).min()
    gy = np.random.default_rng(seed + 1).normal(0.0, 1.0, (m, c)).astype(np.float32)
    return {"mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta, "coef": coef, "h": h, "gy": gy, "z": z, "batch_stats": True}


def _bwd_from_y(case, act, train_bn, with_coef, inplace, misses):
    _abi, L = _lib()
    m, c = case["h"].shape
    y32 = R.act_fwd(case["z"], act).astype(np.float32)               # the fp32 forward value of the same z
    gy, y = _dev(case["gy"]), _dev(y32)
    h = _dev(case["h"]) if train_bn else None
    mean = _dev(case["mean"]) if train_bn else None
    invstd = _dev(case["invstd"]) if train_bn else None
    coef = _dev(case["coef"]) if (train_bn or with_coef) else None
    sums = torch.zeros(2, c, dtype=torch.float64, device="cuda") if train_bn else None
    gbias = torch.zeros(c, dtype=torch.float64, device="cuda")
    gh = gy if inplace else _nan((m, c))
    _abi.check(L.gsn_bn_act_bwd_hip(m, c, gy.data_ptr(), y.data_ptr(), _p(h), _p(mean), _p(invstd), _p(coef), train_bn, act, _p(sums), gh.data_ptr(),
                                    gbias.data_ptr(), _abi.current_stream()), "gsn_bn_act_bwd_hip")
    a = R.adjoint(case["gy"], case["h"], case["mean"], case["invstd"], case["coef"] if coef is not None else None, None, act, train_bn, y=y32,
                  sums=None if sums is None else _np(sums))
    _check_adjoint(a, _np(gh), None if sums is None else _np(sums), _np(gbias), train_bn,
                   "from y %d x %d act %d train_bn %d%s%s" % (m, c, act, train_bn, "" if coef is not None else " no coef", " in place" if inplace else ""), misses,
                   batch_stats=case.get("batch_stats", False))


@pytest.mark.parametrize("m,c", COL_SHAPES + [(65601, 4)])
def test_bn_act_bwd_from_y(m, c):
    """gsn_bn_act_bwd_hip: train_bn 0 with coef null and given, train_bn 1 and 2, every activation; one case in place (grad_h may alias grad_y);
    train_bn 1 also on the batch statistics of the rows themselves."""
    case = R.make_case(m, c, _seed(m, c, 11))
    batch = _batch_case(m, c, _seed(m, c, 13))
    misses = []
    for act in range(4):
        _bwd_from_y(batch, act, 1, True, False, misses)
        _bwd_from_y(case, act, 0, False, False, misses)
        _bwd_from_y(case, act, 0, True, False, misses)
        _bwd_from_y(case, act, 1, True, False, misses)
        _bwd_from_y(case, act, 2, True, False, misses)
    _bwd_from_y(case, 2, 1, True, True, misses)
    assert not misses, misses


def _bwd_from_h(case, act, train_bn, misses):
    _abi, L = _lib()
    m, c = case["h"].shape
    gy, h = _dev(case["gy"]), _dev(case["h"])
    mean, invstd, coef, shift = (_dev(case[k]) for k in ("mean", "invstd", "coef", "beta"))
    sums = torch.zeros(2, c, dtype=torch.float64, device="cuda")
    gbias = torch.zeros(c, dtype=torch.float64, device="cuda")
    gh = _nan((m, c))
    _abi.check(L.gsn_bn_act_bwd_from_h_hip(m, c, gy.data_ptr(), h.data_ptr(), mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), shift.data_ptr(),
                                           train_bn, act, sums.data_ptr(), gh.data_ptr(), gbias.data_ptr(), _abi.current_stream()),
               "gsn_bn_act_bwd_from_h_hip")
    a = R.adjoint(case["gy"], case["h"], case["mean"], case["invstd"], case["coef"], case["beta"], act, train_bn, sums=_np(sums))
    _check_adjoint(a, _np(gh), _np(sums), _np(gbias), train_bn, "from h %d x %d act %d train_bn %d" % (m, c, act, train_bn), misses,
                   batch_stats=case.get("batch_stats", False))


@pytest.mark.parametrize("m,c", COL_SHAPES + [(65601, 4)])
def test_bn_act_bwd_from_h(m, c):
    """gsn_bn_act_bwd_from_h_hip: the activation derivative from z recomputed out of the pre-BatchNorm rows; train_bn 1 and 2, every activation;
    train_bn 1 also on the batch statistics of the rows themselves."""
    misses = []
    for case, modes in ((R.make_case(m, c, _seed(m, c, 12)), (1, 2)), (_batch_case(m, c, _seed(m, c, 14)), (1,))):
        for act, train_bn in itertools.product(range(4), modes):
            _bwd_from_h(case, act, train_bn, misses)
    assert not misses, misses


# ----------------------------------------------------------------------------------------------------------------------
# the plane kernels and the row scratch they write
# ----------------------------------------------------------------------------------------------------------------------
def _scratch(m, c):
    _abi, L = _lib()
    n = int(L.gsn_linear_f16x3_scratch_bytes(m, c))
    assert n == R.scratch_bytes(m, c) and int(L.gsn_linear_f16x3_mpad(m)) == R.mpad(m) and int(L.gsn_linear_f16x3_kpad(c)) == R.kpad(c)
    return _nan((n,), torch.uint8)


def _check_scratch(scr, m, c, ref, slack, key, tag):
    """rowinv an exact power of two below m and exactly 0 from m to m_pad; the row's largest scaled magnitude in [2^14, 2^15] (unless the row
    is zero); every plane half of the padding rows and columns +0; decoded values within
    slack + 2^-22 rowmax of ``ref``.  Returns the worst decoded error in units of that bar."""
    rowinv, hi, lo, val = R.decode_scratch(scr, m, c)
    man, _ = np.frexp(rowinv[:m].astype(np.float64))
    assert np.all(np.isfinite(rowinv[:m])) and np.all(man == 0.5), "rowinv is not a power of two"
    assert not rowinv[m:].view(np.uint32).any(), "rowinv past the rows is not +0"
    assert not hi[m:].view(np.uint16).any() and not lo[m:].view(np.uint16).any(), "padding rows hold something else than +0"
    assert not hi[:, c:].view(np.uint16).any() and not lo[:, c:].view(np.uint16).any(), "padding columns hold something else than +0"
    scaled = np.abs(hi[:m].astype(np.float64) + lo[:m].astype(np.float64)).max(1)
    # (a row of zero planes -- relu with every z < 0; one row under its own batch statistics -- has nothing to scale: the comparison of the
    #  values below says whether zero is right)
    assert np.all((scaled[scaled > 0] >= 2.0 ** 14) & (scaled[scaled > 0] <= 2.0 ** 15)), "a row's largest scaled magnitude is outside [2^14, 2^15]"
    rowmax = np.abs(ref).max(1)
    u = (np.abs(val[:m, :c] - ref) / (slack + 2.0 ** -22 * rowmax[:, None] + 1e-300)).max()
    print("bn-bars planes %s: decoded %.3f of 1" % (tag, _note(key, u)))
    return u


def _fwd_planes(case, act, has=(True, True, True), with_out=True):
    _abi, L = _lib()
    m, c = case["h"].shape
    h = _dev(case["h"])
    vec = [_dev(case[k]) if on else None for k, on in zip(("mean", "coef", "beta"), has)]
    out = _nan((m, c)) if with_out else None
    scr = _scratch(m, c)
    _abi.check(L.gsn_bn_act_planes_hip(m, c, h.data_ptr(), _p(vec[0]), _p(vec[1]), _p(vec[2]), act, _p(out), scr.data_ptr(), _abi.current_stream()),
               "gsn_bn_act_planes_hip")
    return out, scr


@pytest.mark.parametrize("m,c", PLANE_SHAPES + [(65601, 4)])
def test_bn_act_planes_forward(m, c):
    """gsn_bn_act_planes_hip: the fp32 ``out`` at the forward bar, the scratch decoded, and the scratch bit for bit against
    gsn_linear_f16x3_split_rows_hip over the kernel's own ``out`` (the same split of the same values); with and without ``out``."""
    _abi, L = _lib()
    case = R.make_case(m, c, _seed(m, c, 21))
    for act in range(4):
        out, scr = _fwd_planes(case, act)
        u = _note("forward (bar 8)", _forward_units(_np(out), case["h"], case["mean"], case["coef"], case["beta"], act))
        print("bn-bars forward planes %d x %d act %d: %.3f of 8" % (m, c, act, u))
        assert u <= 8.0
        ref, mag = R.forward(case["h"], case["mean"], case["coef"], case["beta"], act)
        assert _check_scratch(scr, m, c, ref, 8.0 * E * mag, "plane decode, forward (bar 1)", "forward %d x %d act %d" % (m, c, act)) <= 1.0
        one = (_abi.gsn_block * 1)()
        one[0].data = out.data_ptr(); one[0].idx = None; one[0].idx32 = None; one[0].width = c
        twin = _scratch(m, c)
        _abi.check(L.gsn_linear_f16x3_split_rows_hip(m, 1, one, twin.data_ptr(), _abi.current_stream()), "gsn_linear_f16x3_split_rows_hip")
        assert torch.equal(scr, twin), "the scratch differs from the row pre-pass over the kernel's own out"
        if act == 1:
            _, alone = _fwd_planes(case, act, with_out=False)
            assert torch.equal(scr, alone), "the scratch depends on whether out is given"


def test_bn_act_planes_forward_with_absent_vectors():
    m, c = 65, 36
    for i, has in enumerate(itertools.product((False, True), repeat=3)):
        if all(has):
            continue
        case = R.make_case(m, c, _seed(m, c, 30 + i), *has)
        out, scr = _fwd_planes(case, 2, has)
        args = [case[k] if on else None for k, on in zip(("mean", "coef", "beta"), has)]
        assert _note("forward (bar 8)", _forward_units(_np(out), case["h"], args[0], args[1], args[2], 2)) <= 8.0
        ref, mag = R.forward(case["h"], args[0], args[1], args[2], 2)
        assert _check_scratch(scr, m, c, ref, 8.0 * E * mag, "plane decode, forward (bar 1)", "forward, vectors %s" % (has,)) <= 1.0


def _bwd_planes(case, act, train_bn, gy=None):
    _abi, L = _lib()
    m, c = case["h"].shape
    gyt, h = _dev(case["gy"] if gy is None else gy), _dev(case["h"])
    mean, invstd, coef, shift = (_dev(case[k]) for k in ("mean", "invstd", "coef", "beta"))
    sums = torch.zeros(2, c, dtype=torch.float64, device="cuda")
    gbias = torch.zeros(c, dtype=torch.float64, device="cuda")
    scr = _scratch(m, c)
    _abi.check(L.gsn_bn_act_bwd_planes_hip(m, c, gyt.data_ptr(), h.data_ptr(), mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), shift.data_ptr(),
                                           train_bn, act, sums.data_ptr(), scr.data_ptr(), gbias.data_ptr(), _abi.current_stream()),
               "gsn_bn_act_bwd_planes_hip")
    return scr, _np(sums), _np(gbias)


def _bwd_planes_checked(case, act, train_bn, misses):
    m, c = case["h"].shape
    scr, sums, gbias = _bwd_planes(case, act, train_bn)
    a = R.adjoint(case["gy"], case["h"], case["mean"], case["invstd"], case["coef"], case["beta"], act, train_bn, sums=sums)
    tag = "adjoint planes %d x %d act %d train_bn %d" % (m, c, act, train_bn)
    assert _check_scratch(scr, m, c, a["gh"], 16.0 * E * a["bound"], "plane decode, adjoint (bar 1)", tag) <= 1.0
    _check_sums(sums, a, misses, tag)
    if train_bn == 1:
        assert not gbias.any()                       # (written analytically: exactly zero, whatever the vectors)
        if case.get("batch_stats"):                  # ... and zero is right, at the column kernels' bar, on batch statistics
            _bar(misses, tag, "bias gradient, batch statistics", (np.abs(a["g_bias"]) / (E * a["g_bias_abs"])).max(), 16.0)
    else:
        assert np.abs(gbias - case["coef"].astype(np.float64) * sums[0]).max() <= 2.0 ** -52 * np.abs(gbias).max()       # = coef * S1
        eb = np.abs(gbias - a["g_bias"])
        _bar(misses, tag, "bias gradient", (eb / (E * np.abs(a["gh"]).sum(0) + TINY)).max(), 8.0, (eb / (8.0 * E * a["g_bias_abs"])).max())


@pytest.mark.parametrize("m,c", PLANE_SHAPES + [(65601, 4)])
def test_bn_act_bwd_planes(m, c):
    """gsn_bn_act_bwd_planes_hip: gH read back from the row scratch, the sums, and the analytic bias gradient (zero under batch statistics,
    coef * S1 on running ones).  Vectors drawn independently of the rows (train_bn 1 and 2), and train_bn 1 on the rows' own batch statistics --
    the setting the entry is for, and the one in which zero IS the bias gradient."""
    misses = []
    for case, modes in ((R.make_case(m, c, _seed(m, c, 22)), (1, 2)), (_batch_case(m, c, _seed(m, c, 24)), (1,))):
        for act, train_bn in itertools.product(range(4), modes):
            _bwd_planes_checked(case, act, train_bn, misses)
    assert not misses, misses


@pytest.mark.parametrize("m", [1, 2, 3])
def test_saturated_units_keep_the_relative_accuracy_of_the_sums(m):
    """Regression (first seen at 1 x 4 and 2 x 8, tanh, through gsn_bn_act_bwd_planes_hip: 32.7 and 19.2 units of the sums' bar of 8, then 8.5
    with an accurate sech^2 of the ROUNDED z).  The activation derivative of a saturated unit is small:
      * 1 - tanhf(z)^2, 1 - y * y and expm1f(z) + 1 round against 1, an absolute 2^-24 where the bar asks for a few 2^-24 of |gZ|: the kernels
        form sech^2 z from e^(-2|z|), (1 - y)(1 + y) and e^z;
      * from h, sech^2 (e^z) answers the fp32 rounding dz of z = (h - mean) coef + shift with a relative error 2 |tanh z| dz (dz), up to
        4 |z| units: act_grad_from_h puts back what the roundings of z dropped, to first order.
    Few rows, |z| in 3 .. 7 (tanh' down to 3e-6, elu' down to 1e-3), every adjoint entry at the stated bars."""
    c, misses = 8, []
    case = R.make_case(m, c, _seed(m, c, 60), z_min=3.0)
    for act, train_bn in itertools.product((2, 3), (1, 2)):
        _bwd_from_y(case, act, train_bn, True, False, misses)
        _bwd_from_h(case, act, train_bn, misses)
        _bwd_planes_checked(case, act, train_bn, misses)
    assert not misses, misses


def _other_rows_untouched(scr, base, m, c, bad):
    r1, h1, l1, _ = R.decode_scratch(scr, m, c)
    r0, h0, l0, _ = R.decode_scratch(base, m, c)
    keep = np.ones(r0.shape[0], dtype=bool)
    keep[bad] = False
    assert np.isnan(r1[bad]).all(), "the inverse scale of a row with an Inf / NaN is not NaN"
    assert np.array_equal(r1[keep].view(np.uint32), r0[keep].view(np.uint32))
    assert np.array_equal(h1[keep].view(np.uint16), h0[keep].view(np.uint16)) and np.array_equal(l1[keep].view(np.uint16), l0[keep].view(np.uint16))


def test_a_non_finite_row_gets_a_nan_inverse_scale_and_every_other_row_is_untouched():
    """one row with an Inf and one with a NaN among finite rows, forward (in h) and adjoint on running statistics (in gY; under batch statistics
    a non-finite gY reaches every row through the column sums, as it does in the mathematics)"""
    m, c, bad = 70, 36, [5, 40]
    case = R.make_case(m, c, _seed(m, c, 23))
    out0, scr0 = _fwd_planes(case, 0)
    poisoned = dict(case)
    poisoned["h"] = case["h"].copy()
    poisoned["h"][5, 7] = np.inf
    poisoned["h"][40, 35] = np.nan
    out1, scr1 = _fwd_planes(poisoned, 0)
    _other_rows_untouched(scr1, scr0, m, c, bad)
    keep = [r for r in range(m) if r not in bad]
    assert torch.equal(out0[keep], out1[keep])
    base, _, _ = _bwd_planes(case, 0, 2)
    gy = case["gy"].copy()
    gy[5, 0] = -np.inf
    gy[40, 20] = np.nan
    scr, _, _ = _bwd_planes(case, 0, 2, gy=gy)
    _other_rows_untouched(scr, base, m, c, bad)


# ----------------------------------------------------------------------------------------------------------------------
# the [2][C] statistics and their producers
# ----------------------------------------------------------------------------------------------------------------------
def _stats_units(stats, rows, m, start=None):
    """worst error of (sum, sum of squares) in units of M 2^-53 (sum |x|, sum x^2) against float64 sums of ``rows``"""
    x = R.f64(rows)
    s0 = np.zeros((2, x.shape[1])) if start is None else start
    err1 = np.abs(stats[0] - (s0[0] + x.sum(0))) / (m * 2.0 ** -53 * np.abs(x).sum(0) + 1e-300)
    err2 = np.abs(stats[1] - (s0[1] + (x * x).sum(0))) / (m * 2.0 ** -53 * (x * x).sum(0) + 1e-300)
    return max(err1.max(), err2.max())


@pytest.mark.parametrize("m", [1, 127, 128, 129, 4099])
@pytest.mark.parametrize("c", [1, 65, 300])
def test_column_stats_adds_float64_sums(m, c):
    """gsn_column_stats_hip (128-row bands, one atomic pair per column and band): ``stats`` starts from non-zero values and is added to.  The
    rows are fp32 values on a 2^-20 grid and the start values multiples of 1/8, so every partial sum is exact in fp64 in any order: the bar
    M 2^-53 (sum |x|, sum x^2) is met only by the exact sums -- a row left out or taken twice shows."""
    _abi, L = _lib()
    rng = np.random.default_rng(_seed(m, c, 31))
    x = (np.round(rng.normal(0.3, 1.0, (m, c)) * 2.0 ** 20) / 2.0 ** 20).astype(np.float32)
    start = np.round(rng.normal(0, 8, (2, c)) * 8) / 8 + 0.125
    stats, h = _dev(start), _dev(x)
    _abi.check(L.gsn_column_stats_hip(m, c, h.data_ptr(), stats.data_ptr(), _abi.current_stream()), "gsn_column_stats_hip")
    u = _note("column statistics (bar 1)", _stats_units(_np(stats), x, m, start))
    print("bn-bars column_stats %d x %d: %.3f of 1" % (m, c, u))
    assert u <= 1.0


@pytest.mark.parametrize("wide", [False, True])
def test_f16x3_product_statistics_are_the_sums_of_the_rows_it_wrote(wide, monkeypatch, capfd):
    """gsn_linear_f16x3_fwd_stats_hip through _dense._linear_hip(..., stats=): the 128 x 128 instantiation and the 128 x 320 one (which takes a
    product of 512 row tiles and more: the smallest such shape)."""
    from gsn_amd import _dense
    m, k, n = (65413, 32, 260) if wide else (6200, 32, 132)
    torch.manual_seed(m)
    x = torch.randn(m, k, device="cuda") + 0.25
    W = torch.randn(n, k, device="cuda") / k ** 0.5
    b = torch.randn(n, device="cuda")
    stats = torch.zeros(2, n, dtype=torch.float64, device="cuda")
    monkeypatch.setenv("GSN_CHAIN_TRACE", "1")
    if wide:
        monkeypatch.setenv("GSN_L16_WIDE", "1")
    capfd.readouterr()
    y = _dense._linear_hip([(x, None)], W, b, None, None, None, 0, m, out=True, stats=stats)
    torch.cuda.synchronize()
    assert "linear_f16x3_kernel (128 x %d tiles)" % (320 if wide else 128) in capfd.readouterr().err
    ref = x[:4096].double() @ W.double().t() + b.double()
    assert ((y[:4096].double() - ref).abs() / ref.abs().amax(1, keepdim=True)).max().item() <= 2e-6      # (the product's own bar, test_wgrad16_gpu.py)
    yd = y.double()
    st = torch.stack([yd.sum(0), (yd * yd).sum(0)])
    mag = torch.stack([yd.abs().sum(0), (yd * yd).sum(0)])
    u = _note("column statistics (bar 1)", ((stats - st).abs() / (m * 2.0 ** -53 * mag)).max().item())
    print("bn-bars f16x3 statistics %s: %.3f of 1" % ("128 x 320" if wide else "128 x 128", u))
    assert u <= 1.0


def test_chain_and_linear_statistics_match_the_float64_product():
    """the statistics of gsn_mlp_chain_fwd_hip and of csrc/linear.hip through _dense._launch_stages(..., stats=): no rows are written, so the
    bar is the one their product tests use (test_layers_gpu.py: rtol 1e-5, atol 1e-5 M); linear.hip with rows: the tight bar on those rows."""
    from gsn_amd._dense import _Stage, _chain_fits, _launch_stages, _linear_hip
    torch.manual_seed(5)
    m = 333
    x = torch.randn(m, 40, device="cuda") + 0.5
    w0, b0 = torch.randn(100, 40, device="cuda") / 40 ** 0.5, torch.randn(100, device="cuda")
    w1, b1 = torch.randn(33, 100, device="cuda") / 10.0, torch.randn(33, device="cuda")
    chain = [_Stage(w0, b0, None, "relu", [(x, None)]), _Stage(w1, b1, None, "identity", ())]
    assert _chain_fits(chain)
    stats = torch.zeros(2, 33, dtype=torch.float64, device="cuda")
    _launch_stages(chain, m, stats=stats)
    hl = torch.relu(x.double() @ w0.double().t() + b0.double()) @ w1.double().t() + b1.double()
    assert torch.allclose(stats[0], hl.sum(0), rtol=1e-5, atol=1e-5 * m) and torch.allclose(stats[1], (hl * hl).sum(0), rtol=1e-5, atol=1e-5 * m)
    # one stage outside the chain kernel (K = 300): csrc/linear.hip, statistics alone
    xk = torch.randn(m, 300, device="cuda") + 0.5
    wk, bk = torch.randn(70, 300, device="cuda") / 300 ** 0.5, torch.randn(70, device="cuda")
    single = [_Stage(wk, bk, None, "identity", [(xk, None)])]
    assert not _chain_fits(single)
    stats = torch.zeros(2, 70, dtype=torch.float64, device="cuda")
    _launch_stages(single, m, stats=stats)
    hk = xk.double() @ wk.double().t() + bk.double()
    assert torch.allclose(stats[0], hk.sum(0), rtol=1e-5, atol=1e-5 * m) and torch.allclose(stats[1], (hk * hk).sum(0), rtol=1e-5, atol=1e-5 * m)
    # the same product with its rows: the sums of the rows it wrote
    stats = torch.zeros(2, 70, dtype=torch.float64, device="cuda")
    y = _linear_hip([(xk, None)], wk, bk, None, None, None, 0, m, out=True, stats=stats)
    u = _note("column statistics (bar 1)", _stats_units(_np(stats), _np(y), m))
    print("bn-bars linear.hip statistics with rows: %.3f of 1" % u)
    assert u <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the finalize entries
# ----------------------------------------------------------------------------------------------------------------------
EPS_BN = 1e-5


def _stage_rows(m, c, seed, affine=True):
    """rows whose NORMALISED values (batch statistics, gamma, beta) keep |z| >= 1e-3: drawn with the batch mean and invstd in the ranges of
    R.make_case, then the offenders pushed away and the statistics taken again until none is left.  One row: z = beta.  Returns (h fp32, gamma, beta, the float64 [2][C] sums of h)."""
    for attempt in range(20):
        rng = np.random.default_rng(seed + 1000003 * attempt)
        gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32) if affine else None
        beta = rng.normal(0.0, 0.5, c)
        beta = (np.where(beta < 0, beta - 0.01, beta + 0.01)).astype(np.float32) if affine else None
        xhat = rng.normal(0.0, 1.0, (m, c))
        if m > 1:                       # standardised per column: the batch mean ~ N(0, 2) and invstd in [0.2, 5] are the ones drawn here
            xhat = (xhat - xhat.mean(0)) / xhat.std(0)
        h = (rng.normal(0.0, 2.0, c) + xhat / rng.uniform(0.2, 5.0, c)).astype(np.float32)
        for _ in range(30):
            h64 = h.astype(np.float64)
            stats = np.stack([h64.sum(0), (h64 * h64).sum(0)])
            v = R.bn_vectors(stats, m, EPS_BN, gamma, beta)
            z = (h64 - v["mean"]) * v["scale"] + v["shift"]
            bad = np.abs(z) < R.Z_MIN_DRAWN
            if not bad.any() or m == 1:
                break
            push = np.broadcast_to(8.0 * R.Z_MIN_DRAWN / np.abs(v["scale"]), h.shape)
            h[bad] += (np.where(z < 0, -push, push))[bad].astype(np.float32)
        if not bad.any() and (affine or m > 1):
            return h, gamma, beta, stats
    raise AssertionError("no rows with |z| >= 1e-3 found")


def _within_ulps(got, ref, n=2):
    return np.all(np.abs(got.astype(np.float64) - ref) <= n * R.ulp32(ref))


def _finalize(entry, m, c, stats, gamma, beta, running, momentum, nbt=None, rows=None, act=0):
    """one call of gsn_bn_finalize_{count,hip,act}; returns the four vectors [4][C] (and the rows of the row pass)"""
    _abi, L = _lib()
    vec = _nan((4, c))
    p0 = vec.data_ptr()
    st = _dev(stats)
    g, b = _dev(gamma), _dev(beta)
    head = (c, m, EPS_BN, float(momentum), st.data_ptr(), _p(g), _p(b), _p(running[0]) if running else None, _p(running[1]) if running else None,
            p0, p0 + 4 * c, p0 + 8 * c, p0 + 12 * c)
    out = None
    if entry == "hip":
        rc = L.gsn_bn_finalize_hip(*head, _abi.current_stream())
    elif entry == "count":
        rc = L.gsn_bn_finalize_count_hip(*head, _p(nbt), _abi.current_stream())
    else:
        out = _nan(tuple(rows.shape))
        rc = L.gsn_bn_finalize_act_hip(*head, _p(nbt), rows.data_ptr(), act, out.data_ptr(), _abi.current_stream())
    _abi.check(rc, "gsn_bn_finalize_" + entry)
    return _np(vec), out


# (one row without beta is left out: z = 0 for every element there, and the condition on z cannot hold)
FINALIZE_CASES = [(m, c, a) for m, c in ((1, 3), (2, 3), (2, 130), (65, 1), (65, 63), (65, 64), (65, 65), (65, 130), (257, 3), (16401, 130), (16401, 8))
                  for a in (True, False) if m > 1 or a]


@pytest.mark.parametrize("m,c,affine", FINALIZE_CASES)
def test_finalize_entries_against_float64_bookkeeping(m, c, affine):
    """Two successive batches (momentum 0.1, then 1.0) through gsn_bn_finalize_count_hip: the four vectors and the running statistics within 2 fp32
    ulp of the float64 bookkeeping from the same sums (unbiased factor M / (M - 1); 1 at M = 1, which only the ABI accepts).  gsn_bn_finalize_hip
    and gsn_bn_finalize_act_hip write the same vectors and running statistics bit for bit; the counter rises by one per call; the row pass of
    bn_finalize_act_kernel (16 401 rows: 1024 row blocks x 4 waves walk 5 strides) at the forward bar, from the vectors the kernel wrote."""
    run = {k: [torch.full((c,), 0.25, device="cuda"), torch.full((c,), 1.5, device="cuda")] for k in ("count", "hip", "act")}
    nbt = {k: torch.tensor(7, dtype=torch.int64, device="cuda") for k in ("count", "act")}
    worst = 0.0
    for call, momentum in enumerate((0.1, 1.0)):
        h, gamma, beta, stats = _stage_rows(m, c, _seed(m, c, 40 + call), affine)
        before = [_np(t).astype(np.float64) for t in run["count"]]
        vc, _ = _finalize("count", m, c, stats, gamma, beta, run["count"], momentum, nbt["count"])
        v = R.bn_vectors(stats, m, EPS_BN, gamma, beta)
        for i, k in enumerate(("mean", "invstd", "scale", "shift")):
            assert not np.isnan(vc[i]).any() and _within_ulps(vc[i], v[k]), k
        rm, rv = R.running_update(before[0], before[1], v["mean"], v["var"], m, momentum)
        assert _within_ulps(_np(run["count"][0]), rm) and _within_ulps(_np(run["count"][1]), rv)
        vh, _ = _finalize("hip", m, c, stats, gamma, beta, run["hip"], momentum)
        assert np.array_equal(vh.view(np.uint32), vc.view(np.uint32))
        rows = _dev(h)
        for act in ((2, 1) if call == 0 else (3, 0)):
            use = run["act"] if act >= 2 else None          # (the second activation of a batch: no second update of the running statistics)
            va, out = _finalize("act", m, c, stats, gamma, beta, use, momentum, nbt["act"] if use else None, rows, act)
            assert np.array_equal(va.view(np.uint32), vc.view(np.uint32)), "gsn_bn_finalize_act_hip's vectors differ from gsn_bn_finalize_count_hip's"
            z = R.pre_activation(h, va[0], va[2], va[3])
            assert np.abs(z).min() >= R.Z_MIN_ASSERTED
            worst = max(worst, _forward_units(_np(out), h, va[0], va[2], va[3], act))
        for i in range(2):
            assert torch.equal(run["act"][i], run["count"][i]) and torch.equal(run["hip"][i], run["count"][i])
        assert int(nbt["count"]) == 8 + call and int(nbt["act"]) == 8 + call
    print("bn-bars forward finalize_act %d x %d: %.3f of 8" % (m, c, _note("forward (bar 8)", worst)))
    assert worst <= 8.0


def test_finalize_without_running_statistics_and_without_a_counter():
    """running_* null: the vectors are written as before, the counter still counts; a counter alone null: the running statistics still move"""
    m, c = 65, 130
    h, gamma, beta, stats = _stage_rows(m, c, _seed(m, c, 50))
    run = [torch.full((c,), 0.25, device="cuda"), torch.full((c,), 1.5, device="cuda")]
    nbt = torch.tensor(3, dtype=torch.int64, device="cuda")
    full, _ = _finalize("count", m, c, stats, gamma, beta, run, 0.1, nbt)
    bare, _ = _finalize("count", m, c, stats, gamma, beta, None, 0.1, nbt)
    assert np.array_equal(full.view(np.uint32), bare.view(np.uint32)) and int(nbt) == 5
    kept = [t.clone() for t in run]
    bare_act, out = _finalize("act", m, c, stats, gamma, beta, None, 0.1, None, _dev(h), 1)
    assert np.array_equal(full.view(np.uint32), bare_act.view(np.uint32)) and int(nbt) == 5
    assert torch.equal(kept[0], run[0]) and torch.equal(kept[1], run[1])
    assert _forward_units(_np(out), h, bare_act[0], bare_act[2], bare_act[3], 1) <= 8.0


def test_a_constant_column_has_variance_zero_exactly():
    """all rows 1000.0 and all rows 0, statistics by gsn_column_stats_hip: the variance is exactly 0, invstd = fp32(eps^-1/2), and the row pass
    gives exactly ``shift`` before the activation"""
    _abi, L = _lib()
    m, c = 257, 2
    h = np.zeros((m, c), dtype=np.float32)
    h[:, 0] = 1000.0
    rows = _dev(h)
    stats = torch.zeros(2, c, dtype=torch.float64, device="cuda")
    _abi.check(L.gsn_column_stats_hip(m, c, rows.data_ptr(), stats.data_ptr(), _abi.current_stream()), "gsn_column_stats_hip")
    assert np.array_equal(_np(stats), [[257000.0, 0.0], [257.0e6, 0.0]])
    gamma, beta = np.array([1.25, -0.75], dtype=np.float32), np.array([0.3, -2.0], dtype=np.float32)
    run = [torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")]
    vec, out = _finalize("act", m, c, _np(stats), gamma, beta, run, 1.0, None, rows, 0)
    want = np.float32(1.0 / np.sqrt(np.float64(EPS_BN)))
    assert np.array_equal(vec[0], [1000.0, 0.0]) and np.all(vec[1] == want)
    assert np.array_equal(_np(run[1]), [0.0, 0.0]) and np.array_equal(_np(run[0]), [1000.0, 0.0])
    assert np.array_equal(_np(out), np.broadcast_to(beta, (m, c)))
    plain, _ = _finalize("hip", m, c, _np(stats), gamma, beta, None, 1.0)
    assert np.array_equal(plain.view(np.uint32), vec.view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------
# conditioning of the batch variance
# ----------------------------------------------------------------------------------------------------------------------
COND_PAIRS = ((0.0, 1.0), (10.0, 1.0), (100.0, 1.0), (1000.0, 10.0), (10.0, 0.01), (100.0, 0.01), (1000.0, 0.001), (4096.0, 0.001), (1.0e6, 1.0))


@pytest.mark.parametrize("m", [257, 100003])
def test_batch_variance_conditioning(m):
    """Every producer of the [2][C] statistics evaluates  var = sum x^2 / M - (sum x / M)^2  from fp64 sums of fp32 values: a relative error of
    about kappa M 2^-53 in the variance, kappa = (mean^2 + sigma^2) / (sigma^2 + eps).  Where that is <= 1e-6 the invstd of both HIP paths
    (gsn_column_stats_hip + gsn_bn_finalize_hip; the statistics epilogue behind a one-stage layers.mlp with identity weight, read back from its
    running variance at momentum 1) must agree with a two-pass float64 evaluation of the same fp32 rows to 1e-6 + 2^-23; everywhere else only
    the invariants hold: finite, positive, at most fp32(eps^-1/2).  Prints the table of profiles/bn_conditioning.txt ("bn-cond ...") with
    torch's own fp32 batch_norm beside it."""
    from gsn_amd import layers
    _abi, L = _lib()
    c = len(COND_PAIRS)
    rng = np.random.default_rng(m)
    mean = np.array([p[0] for p in COND_PAIRS])
    sigma = np.array([p[1] for p in COND_PAIRS])
    h = (mean + sigma * rng.normal(0.0, 1.0, (m, c))).astype(np.float32)
    mu2, var2 = R.two_pass(h)
    ref = 1.0 / np.sqrt(var2 + EPS_BN)
    kappa = (mean ** 2 + sigma ** 2) / (sigma ** 2 + EPS_BN)
    provable = kappa * m * 2.0 ** -53 <= 1e-6
    rows = _dev(h)
    # path 1: the statistics pass over materialised rows + the finalize kernel
    stats = torch.zeros(2, c, dtype=torch.float64, device="cuda")
    _abi.check(L.gsn_column_stats_hip(m, c, rows.data_ptr(), stats.data_ptr(), _abi.current_stream()), "gsn_column_stats_hip")
    vec, _ = _finalize("hip", m, c, _np(stats), None, None, None, 0.0)
    path1 = vec[1].astype(np.float64)
    # path 2: the statistics of a product's epilogue (identity weight: the rows themselves), as a training step takes them
    net = layers.mlp(c, c, [c], 0, activation="relu", batch_norm=True).cuda().train()
    with torch.no_grad():
        net.fc[0].weight.copy_(torch.eye(c)); net.fc[0].bias.zero_()
    net.bn[0].momentum = 1.0
    y = net(rows)
    assert torch.isfinite(y).all()
    path2 = 1.0 / np.sqrt(_np(net.bn[0].running_var).astype(np.float64) * (m - 1.0) / m + EPS_BN)
    # torch's own fp32 training-mode batch_norm on the same rows
    t_out, _, t_invstd = torch.native_batch_norm(rows, None, None, None, None, True, 0.0, EPS_BN)
    theirs = _np(t_invstd).astype(np.float64)
    cap = float(np.float32(1.0 / np.sqrt(EPS_BN))) * (1.0 + 2.0 ** -23)
    for j in range(c):
        e1, e2, et = (abs(p[j] - ref[j]) / ref[j] for p in (path1, path2, theirs))
        print("bn-cond M %6d mean %9g sigma %6g kappa %9.3g kappa*M*2^-53 %8.2g %s | invstd rel. error: stats+finalize %8.2g  mlp epilogue %8.2g  torch fp32 %8.2g"
              % (m, mean[j], sigma[j], kappa[j], kappa[j] * m * 2.0 ** -53, "asserted " if provable[j] else "invariant", e1, e2, et))
    for path in (path1, path2):
        assert np.all(np.isfinite(path)) and np.all(path > 0) and np.all(path <= cap)
        assert np.all(np.abs(path[provable] - ref[provable]) <= (1e-6 + 2.0 ** -23) * ref[provable])
    assert provable.sum() == (5 if m == 257 else 4)              # (the first four pairs, and at 257 rows the fifth: recomputed above, checked here)
