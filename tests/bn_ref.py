"""Shared by tests/test_bn_ref_cpu.py and tests/test_bn_kernels_gpu.py: the float64 restatement of one BatchNorm + activation stage
(models_misc.py:52-59: Z = (H - mean) * scale + shift, Y = act(Z)), of its adjoint as the header of csrc/backward.hip states it, of the
BatchNorm1d bookkeeping of csrc/encode.hip (bn_finalize_kernel) and a decoder of the fp16x3 row scratch written from the layout comments of
csrc/linear_f16.hip.  Plain numpy: nothing here imports the package, the GPU tests compare the sizes below with the ABI's own.

Every function takes the fp32 vectors a kernel is given and evaluates in float64 FROM them: a test of one kernel does not recompute its
inputs.  Activation codes: 0 identity, 1 relu, 2 elu, 3 tanh.  Absent vectors (None) mean 0 / scale 1 / shift 0."""
import numpy as np

EPS = 2.0 ** -24          # half an fp32 ulp of 1: the unit of every bar below


def f64(a):
    """numpy float64 copy of a torch tensor / numpy array / None"""
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def act_fwd(z, act):
    if act == 1:
        return np.where(z > 0, z, 0.0)
    if act == 2:
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    if act == 3:
        return np.tanh(z)
    return z.copy()


def act_grad_from_z(z, act):
    if act == 1:
        return (z > 0).astype(np.float64)
    if act == 2:
        return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))
    if act == 3:
        return 1.0 - np.tanh(z) ** 2
    return np.ones_like(z)


def act_grad_from_y(y, act):
    """the same derivative from the stage OUTPUT (elu: d/dz (e^z - 1) = y + 1 for z <= 0)"""
    if act == 1:
        return (y > 0).astype(np.float64)
    if act == 2:
        return np.where(y > 0, 1.0, y + 1.0)
    if act == 3:
        return 1.0 - y * y
    return np.ones_like(y)


def pre_activation(h, mean, scale, shift):
    h = f64(h)
    mu = 0.0 if mean is None else f64(mean)
    sc = 1.0 if scale is None else f64(scale)
    sh = 0.0 if shift is None else f64(shift)
    return (h - mu) * sc + sh


def forward(h, mean, scale, shift, act):
    """(ref, mag): ref = act((h - mean) * scale + shift) and the magnitude |(h - mean) * scale| + |shift| + |ref| the forward bar is stated in"""
    h = f64(h)
    mu = 0.0 if mean is None else f64(mean)
    sc = 1.0 if scale is None else f64(scale)
    sh = 0.0 if shift is None else f64(shift)
    prod = (h - mu) * sc
    ref = act_fwd(prod + sh, act)
    return ref, np.abs(prod) + np.abs(sh) + np.abs(ref)


# ----------------------------------------------------------------------------------------------------------------------
# adjoint of one stage
# ----------------------------------------------------------------------------------------------------------------------
def adjoint(gy, h, mean, invstd, coef, shift, act, train_bn, y=None, sums=None):
    """gZ = gY act', the two column sums S1 = sum_r gZ, S2 = sum_r gZ xhat (xhat = (H - mean) invstd), and
         train_bn 1 (batch statistics):    gH = coef (gZ - S1 / M - xhat S2 / M)         coef = gamma invstd
         train_bn 2 (running statistics):  gH = coef gZ,  the same two sums for gamma / beta
         train_bn 0 (no BatchNorm vectors wanted): gH = coef gZ (coef None: 1), no sums
    act' from ``y`` when given (gsn_bn_act_bwd_hip), else from z = (H - mean) coef + shift (the _from_h and _planes forms).
    ``sums``: the fp64 [2][C] sums the reduce pass handed to the apply pass -- gH is then formed from THEM (the apply kernel by itself: its
    inputs are not recomputed), while s1 / s2 stay the float64 sums the reduce pass is held to.
    Returns a dict: gz, act_grad, s1, s2 (= g_beta, g_gamma), s1_abs, s2_abs (sum_r |term|), gh, bound, g_bias, g_bias_abs (sum_r bound),
    the coef / xhat the value was formed from (gh_coef, xhat), and gz_mag = |gY| max(1, |act'|) with its column sums s1_mag, s2_mag
    (times |xhat|)."""
    gy = f64(gy)
    m_rows = gy.shape[0]
    cf = np.ones(gy.shape[1]) if coef is None else f64(coef)
    if y is not None:
        da = act_grad_from_y(f64(y), act)
    else:
        da = act_grad_from_z(pre_activation(h, mean, coef, shift), act)
    gz = gy * da
    out = {"gz": gz, "act_grad": da}
    m1 = m2 = xhat = None
    if train_bn:
        xhat = (f64(h) - f64(mean)) * f64(invstd)
        t2 = gz * xhat
        out.update(s1=gz.sum(0), s2=t2.sum(0), s1_abs=np.abs(gz).sum(0), s2_abs=np.abs(t2).sum(0))
        out["g_beta"], out["g_gamma"] = out["s1"], out["s2"]
    bound = np.abs(gy) * np.maximum(1.0, np.abs(da))
    out["gz_mag"] = bound                          # what an fp32 gZ is accurate against: tanh' = 1 - t^2 is formed from t with an absolute error
    if train_bn:
        out.update(s1_mag=bound.sum(0), s2_mag=(bound * np.abs(xhat)).sum(0))
    if train_bn == 1:
        given = None if sums is None else f64(sums).reshape(2, -1)
        m1, m2 = (out["s1"] if given is None else given[0]) / m_rows, (out["s2"] if given is None else given[1]) / m_rows
        gh = cf * (gz - m1 - xhat * m2)
        bound = bound + np.abs(m1) + np.abs(xhat * m2)
    else:
        gh = cf * gz
    out["gh"] = gh
    out["gh_coef"], out["xhat"] = cf, xhat
    out["bound"] = np.abs(cf) * bound
    out["g_bias"] = gh.sum(0)
    out["g_bias_abs"] = out["bound"].sum(0)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm1d bookkeeping
# ----------------------------------------------------------------------------------------------------------------------
def f32(a):
    """round to fp32, back in float64: the kernel's (double)(float)x"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def bn_vectors(stats, m_rows, eps, gamma=None, beta=None):
    """from the [2][C] column sums / sums of squares: mean, biased variance clamped at 0, invstd, scale = gamma invstd, shift = beta.
    All float64 (the kernel forms scale in fp32 from the rounded invstd: two roundings, inside the 2 ulp its test allows)."""
    st = f64(stats).reshape(2, -1)
    mu = st[0] / m_rows
    var = np.maximum(st[1] / m_rows - mu * mu, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = invstd * f64(gamma) if gamma is not None else invstd.copy()
    shift = f64(beta) if beta is not None else np.zeros_like(mu)
    return {"mean": mu, "var": var, "invstd": invstd, "scale": scale, "shift": shift}


def running_update(running_mean, running_var, mean, var, m_rows, momentum):
    """nn.BatchNorm1d's update with the unbiased factor M / (M - 1) (1 at M = 1) and bn_finalize_kernel's roundings:
    new = (1 - momentum) old + momentum (double)(float)value.  float64, before the store's rounding."""
    unbiased = f64(var) * (m_rows / (m_rows - 1.0 if m_rows > 1 else 1.0))
    rm = (1.0 - momentum) * f64(running_mean) + momentum * f32(mean)
    rv = (1.0 - momentum) * f64(running_var) + momentum * f32(unbiased)
    return rm, rv


def two_pass(h):
    """(mean, biased variance) straight from the rows, float64, two passes"""
    h = f64(h)
    mu = h.mean(0)
    return mu, ((h - mu) ** 2).mean(0)


def ulp32(x):
    """spacing of fp32 at |x| (float64)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# the fp16x3 row scratch (csrc/linear_f16.hip: "plane layout in memory [row][K slice][high | low][32 halfs]", rowinv[m_pad] in front,
# "rows of a row scratch: m_rows and at least 128 more (zero planes, zero inverse scales), in whole 256-row tiles")
# ----------------------------------------------------------------------------------------------------------------------
def kpad(k):
    k32 = (k + 31) // 32 * 32
    return max(k32, 64)                               # (the matrix kernel keeps two 32-wide slices in flight)


def mpad(m):
    return 0 if m <= 0 else (m + 128 + 255) // 256 * 256


def scratch_bytes(m, k):
    if m <= 0 or k <= 0:
        return 0
    return mpad(m) * 4 + mpad(m) * kpad(k) * 4


def decode_scratch(buf, m_rows, k):
    """buf: the scratch as bytes (numpy uint8 / torch uint8).  Returns (rowinv fp32 [m_pad], hi fp16 [m_pad][k_pad], lo fp16 [m_pad][k_pad],
    values float64 [m_pad][k_pad] = (hi + lo) rowinv)."""
    if hasattr(buf, "detach"):
        buf = buf.detach().cpu().numpy()
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    mp, kp = mpad(m_rows), kpad(k)
    assert buf.size == scratch_bytes(m_rows, k), (buf.size, scratch_bytes(m_rows, k))
    rowinv = buf[:mp * 4].view(np.float32).copy()
    lines = buf[mp * 4:].view(np.float16).reshape(mp, kp // 32, 2, 32)
    hi = lines[:, :, 0, :].reshape(mp, kp).copy()
    lo = lines[:, :, 1, :].reshape(mp, kp).copy()
    with np.errstate(invalid="ignore"):
        values = (hi.astype(np.float64) + lo.astype(np.float64)) * rowinv.astype(np.float64)[:, None]
    return rowinv, hi, lo, values


def encode_scratch(x):
    """The scratch of fp32 rows x [M][K] from the same comments (l16_scale, l16_split2): per row the power-of-two scale that puts its largest
    magnitude into [2^14, 2^15) (biased exponent clamped to 15 .. 254), hi = fp16(v), lo = fp16(v - hi) in fp32; a row with an Inf / NaN gets a
    NaN inverse scale.  Padding rows and columns: +0 planes, inverse scale 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    m, k = x.shape
    mp, kp = mpad(m), kpad(k)
    bits = (x.view(np.uint32) & np.uint32(0x7fffffff)).max(axis=1).astype(np.int64)
    e = np.clip(bits >> 23, 15, 254)
    scale = ((268 - e) << 23).astype(np.uint32).view(np.float32)
    inv = ((e - 14) << 23).astype(np.uint32).view(np.float32).copy()
    inv[bits >= 0x7f800000] = np.float32(np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * scale[:, None]).astype(np.float32)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    lines = np.zeros((mp, kp // 32, 2, 32), dtype=np.float16)
    hp = np.zeros((m, kp), dtype=np.float16); hp[:, :k] = hi
    lp = np.zeros((m, kp), dtype=np.float16); lp[:, :k] = lo
    lines[:m, :, 0, :] = hp.reshape(m, kp // 32, 32)
    lines[:m, :, 1, :] = lp.reshape(m, kp // 32, 32)
    rowinv = np.zeros(mp, dtype=np.float32); rowinv[:m] = inv
    return np.concatenate([rowinv.view(np.uint8), lines.reshape(-1).view(np.uint8)])


# ----------------------------------------------------------------------------------------------------------------------
# inputs of the kernel tests: per-column vectors first, then z away from 0, then h = mean + (z - shift) / coef rounded to fp32 -- the relu
# derivative is a step at 0, and an fp32 / fp64 disagreement about the sign of z would be the test's fault
# ----------------------------------------------------------------------------------------------------------------------
Z_MIN_DRAWN = 1e-3
Z_MIN_ASSERTED = 1e-4


def make_case(m_rows, n_cols, seed, has_mean=True, has_scale=True, has_shift=True, z_min=Z_MIN_DRAWN):
    """fp32 arrays: mean ~ N(0, 2), invstd in [0.2, 5], gamma in +-[0.5, 1.5], beta ~ N(0, 0.5), coef = fp32(gamma invstd), h, gy.  Absent
    vectors take their identity value here and travel as null pointers.  Asserts the condition on z in float64 from the fp32 arrays."""
    rng = np.random.default_rng(seed)
    mean = (rng.normal(0.0, 2.0, n_cols) if has_mean else np.zeros(n_cols)).astype(np.float32)
    invstd = (rng.uniform(0.2, 5.0, n_cols) if has_scale else np.ones(n_cols)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, n_cols) * rng.choice([-1.0, 1.0], n_cols) if has_scale else np.ones(n_cols)).astype(np.float32)
    beta = (rng.normal(0.0, 0.5, n_cols) if has_shift else np.zeros(n_cols)).astype(np.float32)
    coef = (gamma * invstd).astype(np.float32)
    z = rng.normal(0.0, 1.0, (m_rows, n_cols))
    z = np.where(z < 0, z - z_min, z + z_min)                              # (z_min = 3: saturated units, |z| in 3 .. 7)
    h = (mean.astype(np.float64) + (z - beta.astype(np.float64)) / coef.astype(np.float64)).astype(np.float32)
    gy = rng.normal(0.0, 1.0, (m_rows, n_cols)).astype(np.float32)
    z64 = pre_activation(h, mean, coef, beta)
    assert np.abs(z64).min() >= Z_MIN_ASSERTED, np.abs(z64).min()          # a condition on the inputs: nothing is masked out afterwards
    return {"mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta, "coef": coef, "h": h, "gy": gy, "z": z64}
