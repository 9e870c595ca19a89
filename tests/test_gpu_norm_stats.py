"""Batch statistics of the normalised conv units at large mean / std ratios (csrc/norm.hip).

The one-pass variance E[y^2] - E[y]^2 from the conv epilogue's fp32 partials loses about 2^-24 (mean / std)^2 of the
variance per rounding; unetk_norm_finalize given the activations recomputes the ill-conditioned channels from them
(tests/test_norm_stats_host.py restates both on the host).  Every forward path that writes statistic partials runs here
with output channels at mean / std 0 .. 3000, an all-zero channel and exactly constant channels, under batch norm and
instance norm.  The reference is the float64 moments of the y the kernel wrote, so the conv's own rounding drops out.
"""
import math

import pytest
import torch

from oracle import tf_ops

pytestmark = pytest.mark.gpu

RATIOS = (0.0, 1.0, 10.0, 100.0, 1000.0, 3000.0)
CONSTS = (1.1, 300.7)           # non-dyadic: the one-pass variance of such a channel is not 0
IGEMM = "conv3x3_igemm_kernel<"
LIN = "conv3x3_igemm_lin_kernel<"
LIN_PLAIN = LIN + "4, 1, 1, 2, false, false, false, false, false, false>"
LIN_SK = LIN + "2, 2, 2, 2, false, false, true, false, false, false>"
SK = "lin_sk_fixup_kernel<128, 128>"
BF = "conv3x3_igemm_bf16_kernel<"


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return out, ops.profile_read()[1]


def _has(names, sub):
    return any(sub in n for n in names)


def make_inputs(xshape, wshape, seed, live=None, scale_ratio=1.0):
    """x: small integers in [-4, 4], input channel 0 exactly 1.  w: random eighths over every tap and input channel >= 1
    (the spread), plus a centre-tap weight on input channel 0 (the offset: the same value at every pixel, borders
    included).  Output channel 0 is all zero, 1 .. len(CONSTS) are exactly constant, the rest cycle through RATIOS.
    Everything is exact in fp32 (and bf16) and every partial sum of the conv is a multiple of 1/8."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, xshape, generator=g).float()
    x[..., 0] = 1.0
    cin, cout = wshape[-2], wshape[-1]
    w = torch.randint(-2, 3, wshape, generator=g).float() / 8
    w[..., 0, :] = 0
    live = cin if live is None else live
    w[..., live:, :] = 0
    taps = w[..., 0, 0].numel()
    spread = math.sqrt(taps * (live - 1) * (20.0 / 3.0) * (2.0 / 64.0)) if live > 1 else 1.0
    centre = tuple(k // 2 for k in wshape[:-2])
    w[..., :3] = 0
    for j, c in enumerate(CONSTS):
        w[centre + (0, 1 + j)] = c
    for j in range(1 + len(CONSTS), cout):
        r = RATIOS[(j - 1 - len(CONSTS)) % len(RATIOS)] * scale_ratio
        w[centre + (0, j)] = (1 if j % 2 else -1) * round(r * spread * 8) / 8
    if live < cin:
        x[..., live:] = 0
    return x.cuda(), w.cuda()


def check_stats(ops, y, stats, rows, per_sample, eps):
    """Finalize y's partials (with y) under batch / instance norm and check mean, rstd, moving statistics and z against the
    float64 moments of y; twice, bit-equal; unflagged channels bit-equal to the finalize without y."""
    n, c = y.shape[0], y.shape[-1]
    groups = n if per_sample else 1
    y64 = y.double().reshape(groups, -1, c)
    m64, v64 = y64.mean(1), y64.var(1, unbiased=False)
    s64 = v64.sqrt()
    cnt = y64.shape[1]
    gen = torch.Generator(device="cuda").manual_seed(c)
    gamma = torch.rand(c, generator=gen, device="cuda") + 0.5
    beta = torch.randn(c, generator=gen, device="cuda") * 0.3
    decay = 0.5
    d = ops.norm_desc(y.shape, per_sample)

    def run(with_y):
        mm = torch.zeros(c, device="cuda") if not per_sample else None
        mv = torch.zeros(c, device="cuda") if not per_sample else None
        aff = ops.norm_finalize(d, stats, rows, gamma, beta, eps, decay, True, mm, mv, y.device, y=y if with_y else None)
        z = torch.empty_like(y)
        ops.norm_apply_relu(d, y, aff, z)
        torch.cuda.synchronize()
        return aff.clone(), mm, mv, z

    (aff, mm, mv, z), names = _trace(ops, lambda: run(True))
    mean, rstd, scale, shift = aff[0].double(), aff[1].double(), aff[2].double(), aff[3].double()
    assert ((mean - m64).abs() <= 2.0 ** -22 * m64.abs() + 1e-6 * s64).all(), ((mean - m64).abs() / s64.clamp_min(1e-30)).max()
    r64 = 1.0 / torch.sqrt(v64 + eps)
    err_r = ((rstd - r64).abs() / r64).max().item()
    assert err_r <= 1e-5, err_r
    const = v64 == 0
    assert const[:, 0].all() and const[:, 1:1 + len(CONSTS)].all()
    rstd_eps = (1.0 / torch.sqrt(torch.tensor(eps, dtype=torch.float32, device="cuda"))).item()
    assert (aff[1][const] == rstd_eps).all(), aff[1][const]
    if not per_sample:
        ref_mv = decay * v64[0] * cnt / (cnt - 1)
        assert (mv[const[0]] == 0).all(), mv[const[0]]
        assert ((mv.double() - ref_mv).abs() <= 1e-5 * ref_mv).all(), ((mv.double() - ref_mv).abs() / ref_mv.clamp_min(1e-30)).max()
        ref_mm = decay * m64[0]
        assert ((mm.double() - ref_mm).abs() <= 2.0 ** -21 * ref_mm.abs() + 1e-6 * s64[0]).all()
    # z = relu(y * scale + shift), against the float64 normalisation of y
    yg = y.double().reshape(groups, -1, c)
    z64 = torch.relu(gamma.double() * (yg - m64[:, None]) * r64[:, None] + beta.double())
    zg = z.double().reshape(groups, -1, c)
    fused = (yg * scale[:, None]).abs() + shift[:, None].abs()
    bound = 1e-5 * max(1.0, z64.abs().max().item()) + 8 * 2.0 ** -24 * fused
    excess = ((zg - z64).abs() - bound).max().item()
    assert excess <= 0, excess
    # the constant channels: z is relu(beta) up to the rounding of the fused form
    zc = zg[:, :, const[0]] if groups == 1 else None
    if zc is not None:
        assert ((zc - torch.relu(beta.double()[const[0]])).abs() <= 8 * 2.0 ** -24 * fused[:, :, const[0]]).all()
    assert _has(names, "norm_reduce_finalize_kernel(") and _has(names, "norm_refine_kernel("), names
    # repeatable, bit for bit
    aff2, mm2, mv2, z2 = run(True)
    assert torch.equal(aff.view(torch.int32), aff2.view(torch.int32)) and torch.equal(z.view(torch.int32), z2.view(torch.int32))
    if not per_sample:
        assert torch.equal(mv.view(torch.int32), mv2.view(torch.int32)) and torch.equal(mm.view(torch.int32), mm2.view(torch.int32))
    # y = NULL: today's one-pass results; the channels the rule keeps are bit-equal to them
    (aff0, mm0, mv0, _), names0 = _trace(ops, lambda: run(False))
    assert not _has(names0, "norm_refine_kernel("), names0
    keep = (m64 * m64 <= 16.0 * (v64 + eps)) & (s64 > 0)
    flat = aff.view(torch.int32).reshape(4, groups, c)
    flat0 = aff0.view(torch.int32).reshape(4, groups, c)
    assert keep.any()
    assert torch.equal(flat[:, keep], flat0[:, keep])
    if not per_sample:
        assert torch.equal(mv.view(torch.int32)[keep[0]], mv0.view(torch.int32)[keep[0]])
    return m64, s64


def _ratios_reached(m64, s64):
    r = (m64.abs() / s64.clamp_min(1e-30))[s64 > 0]
    assert r.max().item() > 1000 and (r < 0.5).any() and ((r > 50) & (r < 200)).any()


# ------------------------------------------------------------------------------------------------ 2-D producers
# name, (N, H, W, Cin, Cout), dilation, bf16 operands, kernels the forward must launch
CONV2D = [
    ("cfg0_8row", (4, 56, 224, 128, 128), 1, 0, (IGEMM + "2, 2, 2, 2, 1, 1, 0>",)),
    ("cfg0_4row", (1, 16, 48, 128, 128), 1, 0, (IGEMM + "2, 2, 1, 2, 1, 1, 0>",)),
    ("cfg0_16row_l1", (2, 256, 256, 128, 128), 1, 0, (IGEMM + "2, 2, 4, 2, 1, 1, 0>",)),
    ("cfg1", (2, 16, 48, 32, 64), 1, 0, (IGEMM + "4, 1, 1, 2, 1, 1, 0>",)),
    ("cfg2", (2, 16, 48, 32, 32), 1, 0, (IGEMM + "4, 1, 2, 1, 1, 1, 0>",)),
    ("lin", (2, 24, 24, 32, 64), 1, 0, (LIN_PLAIN,)),
    ("lin_streamk", (8, 16, 16, 128, 128), 1, 0, (LIN_SK, SK)),
    ("c3_first_layer", (2, 24, 40, 3, 64), 1, 0, ("conv3x3_c3_mfma_kernel<3, float, false>",)),
    ("direct_first_layer", (2, 20, 36, 3, 32), 1, 0, ("conv3x3_direct_kernel<3, float>",)),
    ("dilation2", (2, 16, 40, 64, 64), 2, 0, (IGEMM + "4, 1, 1, 2, 1, 2, 0>",)),
    ("bf16_operands", (2, 16, 48, 64, 128), 1, 1, (BF,)),
]


@pytest.mark.parametrize("kind", ["batch_norm", "instance_norm"])
@pytest.mark.parametrize("row", CONV2D, ids=[r[0] for r in CONV2D])
def test_conv3x3_stats(ops, row, kind):
    name, (n, h, w, cin, cout), dil, bf16, kernels = row
    x, wt = make_inputs((n, h, w, cin), (3, 3, cin, cout), seed=cin * 7 + cout + h)
    wp = ops.conv3x3_pack(wt, bf16=bf16)[0] if ops.conv_uses_mfma(cin, cout) else wt
    (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(x, wp, cout, True, bf16=bf16, dilation=dil))
    for k in kernels:
        assert _has(names, k), (k, names)
    per_sample = kind == "instance_norm"
    if name == "cfg0_16row_l1" and not per_sample:
        assert rows > 256           # the first level of the row reduction runs
    m64, s64 = check_stats(ops, y, stats, rows, per_sample, 1e-6 if per_sample else 1e-3)
    _ratios_reached(m64, s64)


# ------------------------------------------------------------------------------------------------ 3-D producers
S2D, SUB = "s2d_kernel", "subsample2_stats_kernel"
# name, (N, D, H, W, Cin, Cout, kd, sd, shw), live input channels (None: all), precision, kernels the forward must launch
CONV3D = [
    ("kd3_taps", (1, 3, 8, 40, 32, 64, 3, 1, 1), None, 0, (IGEMM + "4, 1, 1, 2, 1, 1, 1>",)),   # stats on the last tap
    ("kd3_lin", (2, 4, 12, 12, 32, 64, 3, 1, 1), None, 0, (LIN_PLAIN,)),
    ("native_s2", (1, 2, 8, 66, 32, 64, 1, 1, 2), None, 0, (IGEMM + "4, 1, 1, 2, 2, 1, 0>",)),
    ("subsample_s2", (1, 2, 8, 12, 32, 32, 1, 1, 2), None, 0, (SUB,)),
    ("bridge_222", (2, 6, 12, 12, 64, 128, 3, 2, 2), None, 0, (S2D,)),
    ("bf16c", (2, 4, 12, 12, 32, 64, 3, 1, 1), None, 1, (BF,)),
    ("live8", (2, 4, 12, 12, 64, 64, 3, 1, 1), 40, 0, (LIN_PLAIN,)),
]


@pytest.mark.parametrize("kind", ["batch_norm", "instance_norm"])
@pytest.mark.parametrize("row", CONV3D, ids=[r[0] for r in CONV3D])
def test_conv3d_stats(ops, row, kind):
    from boxsegliver_amd import _abi
    name, (n, dd, h, w, cin, cout, kd, sd, shw), live, prec, kernels = row
    x, wt = make_inputs((n, dd, h, w, cin), (kd, 3, 3, cin, cout), seed=cin * 5 + cout + kd + sd * 3 + shw, live=live)
    live8 = None
    if live is not None:
        live8 = (sum(1 << i for i in range((live + 7) // 8)), 0)
    d = ops.conv3d_desc(x.shape, cout, kd, (sd, shw, shw), live8=live8)
    precision = _abi.BF16 if prec else _abi.FP32
    wp = ops.conv3d_pack(wt, precision=precision)[0]
    (y, stats, rows), names = _trace(ops, lambda: ops.conv3d_fwd(x, wp, d, True, precision=precision))
    for k in kernels:
        assert _has(names, k), (k, names)
    per_sample = kind == "instance_norm"
    m64, s64 = check_stats(ops, y, stats, rows, per_sample, 1e-6 if per_sample else 1e-3)
    _ratios_reached(m64, s64)


# ------------------------------------------------------------------------------------------------ units, end to end
def _unit_ref(x, w, gamma, beta, per_sample, eps, dz, mm0, mv0, decay):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = tf_ops.conv_nd_same(x64, w64)
    if per_sample:
        zn = tf_ops.instance_norm(y, g64, b64, eps=eps)
        nmm = nmv = None
    else:
        zn, nmm, nmv = tf_ops.batch_norm(y, g64, b64, mm0.double(), mv0.double(), True, eps=eps, decay=decay)
    z = torch.relu(zn)
    grads = torch.autograd.grad(z, (x64, w64, g64, b64), dz.double())
    return z.detach(), grads, nmm, nmv


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


UNITS = [("2d", (2, 16, 48, 64, 64)), ("3d", (1, 4, 12, 12, 32, 64))]


@pytest.mark.parametrize("ratio", [100.0, 1000.0])
@pytest.mark.parametrize("kind", ["batch_norm", "instance_norm"])
@pytest.mark.parametrize("unit", UNITS, ids=[u[0] for u in UNITS])
def test_unit_forward_backward_at_large_ratio(ops, unit, kind, ratio):
    name, shape = unit
    per_sample = kind == "instance_norm"
    eps = 1e-6 if per_sample else 1e-3
    cin, cout = shape[-2], shape[-1]
    wshape = (3, 3, cin, cout) if name == "2d" else (3, 3, 3, cin, cout)
    x, wt = make_inputs(shape[:-1], wshape, seed=int(ratio) + cout, scale_ratio=ratio / 1000.0)
    # the channels cycle through RATIOS scaled so that the largest is 3 x `ratio`
    g = torch.Generator(device="cuda").manual_seed(7)
    gamma = torch.rand(cout, generator=g, device="cuda") + 0.5
    beta = torch.randn(cout, generator=g, device="cuda") * 0.3
    decay = 0.9
    mm0 = torch.randn(cout, generator=g, device="cuda")
    mv0 = torch.rand(cout, generator=g, device="cuda") + 0.5
    mm, mv = mm0.clone(), mv0.clone()
    spec = ops.NormSpec(kind, eps=eps, decay=decay, training=True)
    xd = x.clone().requires_grad_(True)
    wd = wt.clone().requires_grad_(True)
    gd, bd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    dz = torch.randn(tuple(x.shape[:-1]) + (cout,), generator=g, device="cuda")

    def step():
        if name == "2d":
            return ops.Conv3x3NormRelu.apply(xd, wd, gd, bd, mm, mv, spec, None, None, None, None)
        return ops.Conv3dNormRelu.apply(xd, wd, gd, bd, mm, mv, spec, (1, 1, 1), None)

    z = step()
    grads = torch.autograd.grad(z, (xd, wd, gd, bd), dz)
    z_ref, g_ref, nmm, nmv = _unit_ref(x, wt, gamma, beta, per_sample, eps, dz, mm0, mv0, decay)
    # z: within 1e-5 of its scale plus the rounding of the fused y * scale + shift form
    y_ref = tf_ops.conv_nd_same(x.double(), wt.double())
    axes = tuple(range(1, y_ref.dim() - 1)) if per_sample else tuple(range(y_ref.dim() - 1))
    r64 = 1.0 / torch.sqrt(y_ref.var(axes, unbiased=False, keepdim=True) + eps)
    sc = gamma.double() * r64
    sh = beta.double() - y_ref.mean(axes, keepdim=True) * sc
    bound = 1e-5 * max(1.0, z_ref.abs().max().item()) + 8 * 2.0 ** -24 * ((y_ref * sc).abs() + sh.abs())
    assert ((z.double() - z_ref).abs() - bound).max().item() <= 0
    # gradients: 2e-5, plus the fp32 mean's rounding, which every x-hat (y - mean) rstd of the backward carries
    tol = 2e-5 + 8 * 2.0 ** -24 * ratio
    for got, ref, what in zip(grads, g_ref, ("dx", "dw", "dgamma", "dbeta")):
        assert _rel(got, ref) < tol, (what, _rel(got, ref), tol)
    if not per_sample:
        torch.testing.assert_close(mv.double(), nmv, rtol=1e-5, atol=0)
        torch.testing.assert_close(mm.double(), nmm, rtol=1e-5, atol=1e-6)
    # repeatable
    mm.copy_(mm0)
    mv.copy_(mv0)
    z2 = step()
    grads2 = torch.autograd.grad(z2, (xd, wd, gd, bd), dz)
    assert torch.equal(z, z2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("kind", ["batch_norm", "instance_norm"])
def test_finalize_two_channels(ops, kind):
    """unetk_norm_finalize at C = 2 (N = 2, HW = 16, two stat rows per group): the finalise kernels take any C > 0 and have no
    thread map, so the host path there must not compute one -- C / 4 = 0 channel quads is a division by zero.  Partials of small
    integers (exact in fp32), against their float64 moments at check_stats' bounds."""
    import ctypes
    from boxsegliver_amd import _abi
    per_sample = kind == "instance_norm"
    eps, decay, n, hw, c = (1e-6 if per_sample else 1e-3), 0.5, 2, 16, 2
    groups = n if per_sample else 1
    g = torch.Generator().manual_seed(11)
    y = torch.randint(-4, 5, (n, hw, c), generator=g).double() + torch.tensor([3.0, -1.0], dtype=torch.float64)
    tiles = y.reshape(2 * groups, -1, c)                             # two tiles per statistics group, each group's contiguous
    rows = tiles.shape[0]
    stats = torch.stack([tiles.sum(1), (tiles * tiles).sum(1)]).float().cuda().contiguous()      # [2][rows][C], exact
    gamma = torch.tensor([1.5, -0.75], device="cuda")
    beta = torch.tensor([0.25, -0.5], device="cuda")
    mm, mv = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    out = torch.full((4, groups, c), float("nan"), device="cuda")
    d = ops.norm_desc((n, hw, c), per_sample)
    L = _abi.lib()
    nbytes = L.unetk_norm_finalize_ws_bytes(ctypes.byref(d), rows)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc, names = _trace(ops, lambda: L.unetk_norm_finalize(
        ctypes.byref(d), p(stats), rows, p(gamma), p(beta), eps, decay, 1, p(mm), p(mv), p(out[0]), p(out[1]), p(out[2]),
        p(out[3]), p(ws), nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert rc == 0, rc
    assert _has(names, "norm_reduce_finalize_kernel(") and not _has(names, "norm_refine_kernel("), names
    y64 = y.reshape(groups, -1, c).cuda()
    m64, v64 = y64.mean(1), y64.var(1, unbiased=False)
    s64, r64, cnt = v64.sqrt(), 1.0 / torch.sqrt(v64 + eps), y64.shape[1]
    mean, rstd, scale, shift = (out[i].double() for i in range(4))
    assert (s64 > 0).all()
    assert ((mean - m64).abs() <= 2.0 ** -22 * m64.abs() + 1e-6 * s64).all(), (mean, m64)
    assert ((rstd - r64).abs() / r64).max().item() <= 1e-5
    sc64 = gamma.double() * r64
    assert ((scale - sc64).abs() <= 1e-5 * sc64.abs()).all()
    assert ((shift - (beta.double() - m64 * sc64)).abs() <= 1e-5 * (beta.double().abs() + (m64 * sc64).abs())).all()
    if per_sample:
        assert (mm == 0).all() and (mv == 0).all()               # instance norm keeps no moving statistics
    else:
        ref_mv, ref_mm = decay * v64[0] * cnt / (cnt - 1), decay * m64[0]
        assert ((mv.double() - ref_mv).abs() <= 1e-5 * ref_mv).all()
        assert ((mm.double() - ref_mm).abs() <= 2.0 ** -21 * ref_mm.abs() + 1e-6 * s64[0]).all()
