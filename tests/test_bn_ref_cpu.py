"""tests/bn_ref.py checked against independent statements of the same mathematics, without a GPU: the stage adjoint against float64
torch.autograd over nn.BatchNorm1d + activation, the bookkeeping against nn.BatchNorm1d over two successive batches, the row-scratch decoder
against an encoder written from the same layout comments (csrc/linear_f16.hip)."""
import numpy as np
import pytest
import torch

import bn_ref as R

ACTS = {0: lambda t: t, 1: torch.relu, 2: torch.nn.functional.elu, 3: torch.tanh}


def _rows(m, c, seed):
    rng = np.random.default_rng(seed)
    h = rng.normal(0.5, 2.0, (m, c))
    gy = rng.normal(0.0, 1.0, (m, c))
    return h, gy


@pytest.mark.parametrize("m", [2, 3, 65])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_adjoint_matches_float64_autograd(m, act, affine, train):
    c, eps = 5, 1e-5
    h, gy = _rows(m, c, 1000 * m + 10 * act + affine)
    bn = torch.nn.BatchNorm1d(c, eps=eps, affine=affine).double()
    rng = np.random.default_rng(7)
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(rng.normal(0.5, 1.0, c)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 6.0, c)))
        if affine:
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)))
            bn.bias.copy_(torch.from_numpy(rng.normal(0.0, 0.5, c)))
    bn.train(train)
    if train:
        mean, var = R.two_pass(h)
    else:
        mean, var = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    ht = torch.from_numpy(h).requires_grad_(True)
    y = ACTS[act](bn(ht))
    (y * torch.from_numpy(gy)).sum().backward()
    invstd = 1.0 / np.sqrt(var + eps)
    gamma = bn.weight.detach().numpy() if affine else np.ones(c)
    beta = bn.bias.detach().numpy() if affine else np.zeros(c)
    coef = gamma * invstd
    # the forward value first
    ref, mag = R.forward(h, mean, coef, beta, act)
    assert np.abs(ref - y.detach().numpy()).max() <= 1e-12 * mag.max()
    for from_y in (False, True):
        a = R.adjoint(gy, h, mean, invstd, coef, beta, act, 1 if train else 2, y=ref if from_y else None)
        tol = 1e-10 * (a["bound"].max() + 1.0)
        assert np.abs(a["gh"] - ht.grad.numpy()).max() <= tol
        assert np.all(a["bound"] >= np.abs(a["gh"]) * (1 - 1e-12))            # the magnitude dominates the value it bounds
        if affine:
            assert np.abs(a["g_gamma"] - bn.weight.grad.numpy()).max() <= 1e-10 * (a["s2_abs"].max() + 1.0)
            assert np.abs(a["g_beta"] - bn.bias.grad.numpy()).max() <= 1e-10 * (a["s1_abs"].max() + 1.0)
        assert np.abs(a["g_bias"] - ht.grad.numpy().sum(0)).max() <= 1e-10 * (a["g_bias_abs"].max() + 1.0)
        if train:                                                                # batch statistics absorb a shift of H
            assert np.abs(a["g_bias"]).max() <= 1e-10 * (a["g_bias_abs"].max() + 1.0)


def test_adjoint_without_batchnorm_is_the_activation_derivative_times_coef():
    h, gy = _rows(9, 4, 3)
    y, _ = R.forward(h, None, None, None, 2)
    a = R.adjoint(gy, None, None, None, None, None, 2, 0, y=y)
    ht = torch.from_numpy(h).requires_grad_(True)
    (torch.nn.functional.elu(ht) * torch.from_numpy(gy)).sum().backward()
    assert np.abs(a["gh"] - ht.grad.numpy()).max() <= 1e-12
    coef = np.array([2.0, -1.0, 0.5, 3.0])
    b = R.adjoint(gy, None, None, None, coef, None, 2, 0, y=y)
    assert np.abs(b["gh"] - ht.grad.numpy() * coef).max() <= 1e-12


@pytest.mark.parametrize("m", [2, 3, 65])
@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_bookkeeping_matches_batchnorm1d_over_two_batches(m, momentum):
    c, eps = 6, 1e-5
    bn = torch.nn.BatchNorm1d(c, eps=eps, momentum=momentum).double().train()
    rng = np.random.default_rng(m)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c)))
        bn.bias.copy_(torch.from_numpy(rng.normal(0.0, 0.5, c)))
    rm, rv = np.zeros(c), np.ones(c)
    for batch in range(2):
        h = rng.normal(3.0 * batch, 1.0 + batch, (m, c))
        out = bn(torch.from_numpy(h)).detach().numpy()
        stats = np.stack([h.sum(0), (h * h).sum(0)])
        v = R.bn_vectors(stats, m, eps, bn.weight.detach().numpy(), bn.bias.detach().numpy())
        mu2, var2 = R.two_pass(h)
        assert np.abs(v["mean"] - mu2).max() <= 1e-13 * np.abs(h).max()
        assert np.abs(v["var"] - var2).max() <= 1e-11 * (h * h).max()
        assert np.abs((h - v["mean"]) * v["scale"] + v["shift"] - out).max() <= 1e-9
        rm_new, rv_new = R.running_update(rm, rv, v["mean"], v["var"], m, momentum)
        # (the reference rounds the batch value to fp32 as bn_finalize_kernel does: 2^-24 relative of it, against the float64 module)
        assert np.abs(rm_new - bn.running_mean.numpy()).max() <= 2.0 ** -23 * np.abs(v["mean"]).max() + 1e-12
        assert np.abs(rv_new - bn.running_var.numpy()).max() <= 2.0 ** -23 * np.abs(v["var"]).max() * m / (m - 1) + 1e-12
        rm, rv = rm_new, rv_new
    assert int(bn.num_batches_tracked) == 2


def test_running_update_at_one_row_uses_the_factor_one():
    rm, rv = R.running_update(np.zeros(2), np.ones(2), np.array([3.0, -1.0]), np.array([0.0, 0.25]), 1, 0.5)
    assert np.array_equal(rm, [1.5, -0.5]) and np.array_equal(rv, [0.5, 0.625])


def test_variance_is_clamped_at_zero_and_ulp32_is_the_fp32_spacing():
    v = R.bn_vectors(np.array([[3000.0], [3.0e6 - 1e-6]]), 3, 1e-5)
    assert v["var"][0] == 0.0 and v["invstd"][0] == 1.0 / np.sqrt(1e-5)
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(-3.0) == 2.0 ** -22


def test_sizes_follow_the_layout_comments():
    assert [R.kpad(k) for k in (1, 4, 32, 33, 64, 65, 300, 640)] == [64, 64, 64, 64, 64, 96, 320, 640]
    assert [R.mpad(m) for m in (0, 1, 128, 129, 384, 385)] == [0, 256, 256, 512, 512, 768]
    assert R.scratch_bytes(65, 36) == 256 * 4 + 256 * 64 * 4 and R.scratch_bytes(0, 36) == 0


@pytest.mark.parametrize("m,k", [(1, 4), (5, 36), (33, 64), (130, 100)])
def test_decoder_inverts_the_encoder(m, k):
    rng = np.random.default_rng(m * 1000 + k)
    x = (rng.normal(0, 1, (m, k)) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(np.float32)
    if m >= 5:
        x[0] = 0.0                                           # largest magnitude 0
        x[1] *= np.float32(1e-30) / np.abs(x[1]).max()       # 1e-30
        x[2] *= np.float32(1e30) / np.abs(x[2]).max()        # 1e30
        x[3, 1:] *= np.float32(2.0 ** -20)                   # values far below the row's largest
    buf = R.encode_scratch(x)
    assert buf.size == R.scratch_bytes(m, k)
    rowinv, hi, lo, val = R.decode_scratch(buf, m, k)
    mp, kp = R.mpad(m), R.kpad(k)
    assert rowinv.shape == (mp,) and hi.shape == (mp, kp) and lo.shape == (mp, kp) and val.shape == (mp, kp)
    rowmax = np.abs(x.astype(np.float64)).max(1)
    assert np.all(np.abs(val[:m, :k] - x.astype(np.float64)) <= 2.0 ** -22 * rowmax[:, None])
    # exact powers of two below m, 0 above; zero planes in the padding
    man, _ = np.frexp(rowinv[:m].astype(np.float64))
    assert np.all(man == 0.5) and np.all(rowinv[m:] == 0)
    assert not hi[m:].view(np.uint16).any() and not lo[m:].view(np.uint16).any()
    assert not hi[:, k:].view(np.uint16).any() and not lo[:, k:].view(np.uint16).any()
    scaled = np.abs(hi[:m].astype(np.float64) + lo[:m].astype(np.float64)).max(1)
    nz = rowmax > 0
    assert np.all((scaled[nz] >= 2.0 ** 14) & (scaled[nz] <= 2.0 ** 15)) and np.all(scaled[~nz] == 0)


def test_a_non_finite_row_decodes_to_a_nan_inverse_scale_alone():
    x = np.ones((4, 8), dtype=np.float32)
    x[1, 3] = np.inf
    x[2, 0] = np.nan
    rowinv, _, _, val = R.decode_scratch(R.encode_scratch(x), 4, 8)
    assert np.isnan(rowinv[1]) and np.isnan(rowinv[2]) and rowinv[0] == rowinv[3] == 2.0 ** -14
    assert np.array_equal(val[[0, 3], :8], np.ones((2, 8)))


def test_make_case_keeps_z_away_from_zero_and_honours_absent_vectors():
    c = R.make_case(257, 5, 1)
    assert np.abs(c["z"]).min() >= R.Z_MIN_ASSERTED and c["h"].dtype == np.float32
    d = R.make_case(3, 2, 2, has_mean=False, has_scale=False, has_shift=False)
    assert not d["mean"].any() and np.all(d["coef"] == 1) and not d["beta"].any()
    assert np.array_equal(R.pre_activation(d["h"], None, None, None), d["z"])
