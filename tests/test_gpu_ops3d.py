"""GPU parity of the 3-D conv composition (unetk_conv3d_*) against the CPU oracle: every (kernel, stride)
pair of UNet3D's _ModelConfig (UNet3D.py:31-91), even and odd extents (TF SAME asymmetric padding), the
32-channel tile configurations, forward + norm-statistic partials + input gradient + filter gradient."""
import math

import numpy as np
import pytest
import torch

from oracle import tf_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    return _ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.float32).cuda()


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


CASES = [
    # N, D, H, W, Cin, Cout, kd, (sd, sh, sw)
    (2, 3, 16, 16, 32, 32, 1, (1, 1, 1)),      # conv_e0/conv2, conv_d0: (1,3,3)
    (1, 4, 16, 32, 32, 64, 1, (1, 2, 2)),      # conv_e1/conv1: (1,3,3) stride (1,2,2), even sizes
    (1, 2, 15, 17, 32, 64, 1, (1, 2, 2)),      # odd sizes: pad 1 before
    (2, 4, 8, 16, 64, 64, 3, (1, 1, 1)),       # (3,3,3) stride 1
    (1, 5, 8, 8, 64, 128, 3, (1, 2, 2)),       # conv_e2/conv1: (3,3,3) stride (1,2,2)
    (1, 6, 8, 16, 64, 64, 3, (2, 2, 2)),       # bridge/conv1: (3,3,3) stride (2,2,2), even depth
    (1, 5, 6, 6, 64, 64, 3, (2, 2, 2)),        # odd depth / odd result sizes
    (1, 2, 8, 16, 128, 32, 1, (1, 1, 1)),      # 64 -> 30 style (conv_d0/conv1)
    # small planes -> linear-pixel kernel (conv_igemm_lin.hip): blocks span rows and planes, never samples
    (2, 8, 12, 12, 64, 128, 3, (1, 1, 1)),     # conv_e3 / conv_d3 shape: 1152 pixels per sample = 9 blocks
    (2, 7, 6, 6, 64, 64, 3, (1, 1, 1)),        # bridge shape: 252 pixels per sample (last block partial)
    (1, 5, 24, 24, 32, 64, 3, (1, 1, 1)),      # conv_e2 shape
    (3, 4, 11, 13, 32, 64, 1, (1, 1, 1)),      # odd plane, three samples, (1,3,3)
    # D = 1: depth taps 0 and 2 have no input plane (forward / input gradient: the middle tap alone; dw[0] = dw[2] = 0)
    (1, 1, 8, 16, 64, 64, 3, (1, 1, 1)),       # one filter-gradient tile: one split, dw written in place
    (3, 1, 6, 6, 64, 64, 3, (1, 1, 1)),        # three one-plane samples side by side, stacked-plane filter gradient
    # stride-2 input gradient on dy planes the four-class linear-pixel kernel refuses (unetk_conv_lin_gen_ok: the padded rows
    # of a pixel block pass its LDS bound): dy zero-dilated into the workspace, dx zeroed, one accumulating stride-1 launch
    # per depth tap onto depth-strided dx planes (conv3d.hip DGRAD_DILATED)
    (1, 2, 16, 160, 32, 64, 1, (1, 2, 2)),     # dy 8 x 80: the first stride-2 layer of a 12 x 160 x 160 patch
    (1, 3, 8, 224, 64, 64, 3, (1, 2, 2)),      # dy 4 x 112: 224-wide patches, three depth taps
    (1, 4, 4, 2, 64, 64, 3, (2, 2, 2)),        # dy 2 x 1: a plane narrower than any tile, depth stride 2
]


@pytest.mark.parametrize("case", CASES)
def test_conv3d_forward_backward(ops, case):
    n, dd, h, w, cin, cout, kd, stride = case
    rng = np.random.default_rng(abs(hash(case)) % 2**31)
    x = torch.tensor(rng.standard_normal((n, dd, h, w, cin)), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(rng.standard_normal((kd, 3, 3, cin, cout)) / math.sqrt(9 * kd * cin), dtype=torch.float64,
                      requires_grad=True)
    y_ref = tf_ops.conv_nd_same(x, wt, stride=stride)
    dy = rng.standard_normal(tuple(y_ref.shape))
    y_ref.backward(torch.tensor(dy))
    d = ops.conv3d_desc(x.shape, cout, kd, stride)
    assert ops.conv3d_out_shape(d) == tuple(y_ref.shape)
    wp_f, wp_d = ops.conv3d_pack(dev(wt.detach().numpy()))
    y, stats, rows = ops.conv3d_fwd(dev(x.detach().numpy()), wp_f, d, want_stats=True)
    ref = y_ref.detach().numpy()
    assert rel_err(y.cpu().numpy(), ref) < 3e-6
    s = stats.cpu().numpy().astype(np.float64)
    assert rows % n == 0                                            # each sample's rows are contiguous
    per = s.reshape(2, n, rows // n, cout).sum(2)
    np.testing.assert_allclose(per[0], ref.sum((1, 2, 3)), atol=3e-4 * max(1.0, np.abs(ref).sum((1, 2, 3)).max()))
    np.testing.assert_allclose(per[1], (ref ** 2).sum((1, 2, 3)), rtol=3e-5)
    dx = ops.conv3d_dgrad(dev(dy), wp_d, d)
    assert rel_err(dx.cpu().numpy(), x.grad.numpy()) < 5e-6
    dw = ops.conv3d_wgrad(dev(x.detach().numpy()), dev(dy), d)
    assert rel_err(dw.cpu().numpy(), wt.grad.numpy()) < 5e-6


def _mask8(segs):
    m = 0
    for lo, hi in segs:
        for g in range(lo // 8, (hi + 7) // 8):
            m |= 1 << g
    return m


LIVE_CASES = [
    # N, D, H, W, Cin, live Cin ranges, Cout, live Cout ranges, kd, stride -- UNet3D's channel-padded layers (NetworksV2/padded.py)
    (1, 8, 12, 12, 256, [(0, 240)], 256, [(0, 240)], 3, (1, 1, 1)),                 # 240 in 256: chunk 15 is skipped
    (1, 6, 24, 24, 128, [(0, 120)], 128, [(0, 120)], 3, (1, 1, 1)),                 # 120 in 128: chunk 7 runs half its MFMAs
    (1, 8, 12, 12, 512, [(0, 240), (256, 496)], 256, [(0, 240)], 3, (1, 1, 1)),     # concat(skip, up) of two padded halves
    (1, 4, 24, 24, 256, [(0, 120), (128, 248)], 128, [(0, 120)], 3, (1, 1, 1)),
    (2, 4, 24, 24, 128, [(0, 120)], 256, [(0, 240)], 3, (1, 2, 2)),                 # grouped-tap forward, four-class input gradient
    (1, 8, 12, 12, 256, [(0, 240)], 320, [(0, 320)], 3, (2, 2, 2)),                 # the bridge
    (3, 16, 12, 12, 256, [(0, 240)], 256, [(0, 240)], 3, (1, 1, 1)),                # whole tiles + stream-K remainder
]


@pytest.mark.parametrize("case", LIVE_CASES)
def test_conv3d_live_channel_masks(ops, case):
    """unetk_conv3d_desc.cin_live8 / cout_live8: skipping the padded groups of the contraction axis gives the result of
    contracting their zeros -- against the oracle on the padded tensors and against the same call without the masks."""
    n, dd, h, w, cin, cin_live, cout, cout_live, kd, stride = case
    rng = np.random.default_rng(cin * 7 + cout + h)
    ci = np.zeros(cin, bool)
    co = np.zeros(cout, bool)
    for lo, hi in cin_live:
        ci[lo:hi] = True
    for lo, hi in cout_live:
        co[lo:hi] = True
    x_np = rng.standard_normal((n, dd, h, w, cin)) * ci
    w_np = rng.standard_normal((kd, 3, 3, cin, cout)) / math.sqrt(9 * kd * cin) * ci[:, None] * co[None, :]
    x = torch.tensor(x_np, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w_np, dtype=torch.float64, requires_grad=True)
    y_ref = tf_ops.conv_nd_same(x, wt, stride=stride)
    dy = rng.standard_normal(tuple(y_ref.shape)) * co
    y_ref.backward(torch.tensor(dy))
    live8 = (_mask8(cin_live), _mask8(cout_live))
    d_live = ops.conv3d_desc(x.shape, cout, kd, stride, live8=live8)
    d_all = ops.conv3d_desc(x.shape, cout, kd, stride)
    assert tuple(d_live.cin_live8) == (live8[0] & 0xFFFFFFFF, live8[0] >> 32)
    wp_f, wp_d = ops.conv3d_pack(dev(w_np))
    xd, dyd = dev(x_np), dev(dy)
    y, stats, rows = ops.conv3d_fwd(xd, wp_f, d_live, want_stats=True)
    y0, stats0, rows0 = ops.conv3d_fwd(xd, wp_f, d_all, want_stats=True)
    ref = y_ref.detach().numpy()
    assert rel_err(y.cpu().numpy(), ref) < 3e-6
    assert rel_err(y.cpu().numpy(), y0.cpu().numpy()) < 1e-6
    assert rows == rows0
    np.testing.assert_allclose(stats.cpu().numpy().reshape(2, -1, cout).sum(1), stats0.cpu().numpy().reshape(2, -1, cout).sum(1),
                               rtol=2e-5, atol=2e-3)
    dx = ops.conv3d_dgrad(dyd, wp_d, d_live)
    dx0 = ops.conv3d_dgrad(dyd, wp_d, d_all)
    assert rel_err(dx.cpu().numpy(), x.grad.numpy()) < 5e-6
    assert rel_err(dx.cpu().numpy(), dx0.cpu().numpy()) < 1e-6
    assert float(dx[..., ~torch.as_tensor(ci)].abs().max()) == 0.0 if not ci.all() else True
    # bit-reproducible with the masks as without
    assert torch.equal(ops.conv3d_fwd(xd, wp_f, d_live, want_stats=False)[0], y)
    assert torch.equal(ops.conv3d_dgrad(dyd, wp_d, d_live), dx)
    dw = ops.conv3d_wgrad(xd, dyd, d_live)                          # the filter gradient contracts pixels: masks unused
    assert rel_err(dw.cpu().numpy(), wt.grad.numpy()) < 5e-6


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    launches = []
    for name in ops.profile_read()[1]:
        name = name.replace(" ", "").replace("(anonymousnamespace)::", "").split("(")[0]
        if name.startswith("void"):
            name = name[4:]
        if "pack_" not in name:
            launches.append(name)
    return out, launches           # every launch, in order: a doubled or reordered launch shows


def exact_inputs(case, live=None):
    """The exact-tier operands of exact_case (also the inputs of the 3-D rows of tests/nonfinite_cases.py): float64 x
    [N, D, H, W, Cin] integers in [-4, 4] and w [kd, 3, 3, Cin, Cout] eighths in [-2/8, 2/8], masked to the live channels of a
    channel-padded row.  Returns (x, w, the generator (dy is drawn from it next), the live-Cout mask or None, live8 or None)."""
    n, dd, h, w, cin, cout, kd, stride = case
    g = torch.Generator().manual_seed(n * 1000 + dd * 100 + h + cin + cout + kd)
    x = torch.randint(-4, 5, (n, dd, h, w, cin), generator=g).double()
    wt = torch.randint(-2, 3, (kd, 3, 3, cin, cout), generator=g).double() / 8
    co, live8 = None, None
    if live is not None:
        ci, co = torch.zeros(cin, dtype=torch.bool), torch.zeros(cout, dtype=torch.bool)
        for lo, hi in live[0]:
            ci[lo:hi] = True
        for lo, hi in live[1]:
            co[lo:hi] = True
        x = x * ci
        wt = wt * ci[:, None] * co[None, :]
        live8 = (_mask8(live[0]), _mask8(live[1]))
    return x, wt, g, co, live8


def exact_case(ops, case, live=None):
    """One case with inputs for which fp32 arithmetic is exact in any summation order (x integers in [-4, 4], w eighths in
    [-2/8, 2/8], dy integers in [-2, 2]: tests/test_gpu_conv_paths.py): y, dx, dw must equal float64 bit for bit whatever
    stride-2 tile, depth-tap accumulation, grouped taps, four-class scatter, half chunk or fused depth tap computes them.
    Returns the traced launches (forward, input gradient, filter gradient), in order."""
    n, dd, h, w, cin, cout, kd, stride = case
    x, wt, g, co, live8 = exact_inputs(case, live)
    x.requires_grad_(True)
    wt.requires_grad_(True)
    y_ref = tf_ops.conv_nd_same(x, wt, stride=stride)
    dy = torch.randint(-2, 3, tuple(y_ref.shape), generator=g).double()
    if live is not None:
        dy = dy * co
    y_ref.backward(dy)
    # the exact regime, from this case's own inputs
    with torch.no_grad():
        assert tf_ops.conv_nd_same(x.abs(), wt.abs(), stride=stride).max().item() * 8 < 2 ** 24
    assert 9 * kd * cout * 2 * 0.25 * 8 < 2 ** 24 and 8 * dy.numel() // cout < 2 ** 24
    d = ops.conv3d_desc(x.shape, cout, kd, stride, live8=live8)
    xd, dyd = x.detach().float().cuda(), dy.float().cuda()
    wp_f, wp_d = ops.conv3d_pack(wt.detach().float().cuda())
    (y, stats, rows), t_f = _trace(ops, lambda: ops.conv3d_fwd(xd, wp_f, d, want_stats=True))
    assert torch.equal(y.double().cpu(), y_ref.detach())
    dx, t_d = _trace(ops, lambda: ops.conv3d_dgrad(dyd, wp_d, d))
    assert torch.equal(dx.double().cpu(), x.grad)
    dw, t_w = _trace(ops, lambda: ops.conv3d_wgrad(xd, dyd, d))
    assert torch.equal(dw.double().cpu(), wt.grad)
    assert torch.equal(dw, ops.conv3d_wgrad(xd, dyd, d))
    return t_f, t_d, t_w


# the launches of each case (forward, input gradient, filter gradient) in order, recorded from the launch trace: a case that
# lands elsewhere after a dispatch change fails here instead of quietly testing something else
EXACT_TRACES = {
    0: (['conv3x3_igemm_kernel<4,1,2,1,1,1,0>'],
        ['conv3x3_igemm_kernel<4,1,2,1,1,1,0>'],
        ['conv3x3_wgrad_kernel<32,32,false,8,16,false,1,1>', 'slab_reduce_kernel<4>']),
    1: (['conv3x3_igemm_kernel<4,1,1,2,2,1,0>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,1,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<4>']),
    2: (['conv3x3_igemm_kernel<4,1,1,2,2,1,0>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,1,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<1>']),
    3: (['conv3x3_igemm_kernel<4,1,1,2,1,1,1>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_igemm_kernel<4,1,1,2,1,1,1>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>', 'slab_reduce_kernel<4>']),
    4: (['s2d_kernel', 'conv3x3_igemm_lin_kernel<2,2,2,2,false,false,false,false,true,false>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,2,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<1>']),
    5: (['s2d_kernel', 'conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,true,false>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,2,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<1>']),
    6: (['conv3x3_igemm_kernel<4,1,1,2,2,1,0>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,2,true,true,false,false,false,false>', 'conv3x3_igemm_lin_kernel<4,1,1,2,true,true,false,false,false,false>', 'conv3x3_igemm_lin_kernel<4,1,1,2,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<1>']),
    7: (['conv3x3_igemm_kernel<4,1,2,1,1,1,0>'],
        ['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<64,32,false,8,16,false,1,1>', 'slab_reduce_kernel<1>']),
    8: (['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,64>'],
        ['conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>', 'slab_reduce_kernel<4>']),
    9: (['conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>'],
        ['conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<64,64,false,20,6,true,1,1>', 'slab_reduce_kernel<1>']),
    10: (['conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,64>'],
        ['conv3x3_igemm_kernel<4,1,2,1,1,1,1>', 'conv3x3_igemm_kernel<4,1,2,1,1,1,1>', 'conv3x3_igemm_kernel<4,1,2,1,1,1,1>'],
        ['conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>', 'slab_reduce_kernel<4>']),
    11: (['conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,false,false,false>'],
        ['conv3x3_igemm_kernel<4,1,2,1,1,1,0>'],
        ['conv3x3_wgrad_kernel<32,64,false,8,16,false,1,1>', 'slab_reduce_kernel<4>']),
    12: (['conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_wgrad_kernel<64,64,false,8,16,false,1,1>']),
    13: (['conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_wgrad_kernel<64,64,false,20,6,true,1,1>', 'slab_reduce_kernel<1>']),
    14: (['conv3x3_igemm_kernel<4,1,1,2,2,1,0>'],
        ['dilate2_kernel', 'conv3x3_igemm_kernel<4,1,2,1,1,1,0>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<4>']),
    15: (['conv3x3_igemm_kernel<4,1,1,2,2,1,0>'],
        ['dilate2_kernel', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<4>']),
    16: (['conv3x3_igemm_kernel<4,1,1,2,2,1,0>'],
        ['dilate2_kernel', 'conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,true,false,false>', 'conv3x3_igemm_lin_kernel<4,1,1,2,false,false,false,true,false,false>', 'conv3x3_igemm_kernel<4,1,1,2,1,1,1>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,16,false,2,1>', 'slab_reduce_kernel<1>']),
}
EXACT_LIVE_TRACES = {
    0: (['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>', 'slab_reduce_kernel<1>']),
    1: (['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,true>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,true>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>', 'slab_reduce_kernel<4>']),
    2: (['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>', 'slab_reduce_kernel<1>']),
    3: (['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,true>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,true>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>', 'slab_reduce_kernel<4>']),
    4: (['s2d_kernel', 'conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,true,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<2,2,1,1,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,12,false,2,1>', 'slab_reduce_kernel<4>']),
    5: (['s2d_kernel', 'conv3x3_igemm_lin_kernel<4,1,1,2,false,false,true,false,true,false>', 'lin_sk_fixup_kernel<128,64>'],
        ['conv3x3_igemm_lin_kernel<2,2,1,1,true,true,false,false,false,false>'],
        ['conv3x3_wgrad_kernel<32,64,false,4,6,false,2,1>', 'slab_reduce_kernel<1>']),
    6: (['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_igemm_lin_kernel<2,2,2,2,false,false,true,false,false,false>', 'lin_sk_fixup_kernel<128,128>'],
        ['conv3x3_wgrad_kernel<64,64,false,10,12,true,1,1>', 'slab_reduce_kernel<1>']),
}


@pytest.mark.parametrize("i", range(len(CASES)))
def test_conv3d_exact_inputs(ops, i):
    assert exact_case(ops, CASES[i]) == EXACT_TRACES[i]


@pytest.mark.parametrize("i", range(len(LIVE_CASES)))
def test_conv3d_live_exact_inputs(ops, i):
    n, dd, h, w, cin, cin_live, cout, cout_live, kd, stride = LIVE_CASES[i]
    assert exact_case(ops, (n, dd, h, w, cin, cout, kd, stride), live=(cin_live, cout_live)) == EXACT_LIVE_TRACES[i]


DECONV_CASES = [
    # N, D, H, W, Cin, Cout, kd
    (1, 3, 4, 8, 128, 64, 1),      # conv_d1/up: (1,2,2)
    (2, 2, 8, 8, 64, 32, 1),       # conv_d0/up: 60 -> 30 padded to 64 -> 32
    (1, 2, 3, 4, 320, 256, 2),     # conv_d3/up: (2,2,2)
    (2, 3, 2, 2, 64, 64, 2),
]


@pytest.mark.parametrize("case", DECONV_CASES)
def test_deconv3d_concat_forward_backward(ops, case):
    n, dd, h, w, cin, cout, kd = case
    rng = np.random.default_rng(cin + kd)
    x = torch.tensor(rng.standard_normal((n, dd, h, w, cin)), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(rng.standard_normal((kd, 2, 2, cout, cin)) / math.sqrt(cin), dtype=torch.float64, requires_grad=True)
    skip = rng.standard_normal((n, kd * dd, 2 * h, 2 * w, cout))
    up = torch.relu(tf_ops.conv_transpose_ks(x, wt, (kd, 2, 2)))          # UNet3D: no bias, ReLU
    cat_ref = torch.cat((torch.tensor(skip), up), dim=-1)
    dcat = rng.standard_normal(tuple(cat_ref.shape))
    cat_ref.backward(torch.tensor(dcat))
    cat = torch.zeros((n, kd * dd, 2 * h, 2 * w, 2 * cout), device="cuda")
    cat[..., :cout] = dev(skip)
    wp_f, wp_d = ops.deconv3d_pack(dev(wt.detach().numpy()))
    ops.deconv3d_fwd(dev(x.detach().numpy()), wp_f, None, cat, cout, cout, kd)
    assert rel_err(cat.cpu().numpy(), cat_ref.detach().numpy()) < 3e-6
    dx, dw, db = ops.deconv3d_bwd(dev(x.detach().numpy()), wp_d, cat, dev(dcat), cout, cout, kd, want_dbias=False)
    assert db is None
    assert rel_err(dx.cpu().numpy(), x.grad.numpy()) < 5e-6
    assert rel_err(dw.cpu().numpy(), wt.grad.numpy()) < 5e-6


def test_conv3d_first_layer_single_channel(ops):
    # conv_e0/conv1: Cin = 1 (direct kernel on raw DHWIO filters), Cout = 30 padded to 32
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.standard_normal((2, 3, 16, 32, 1)), dtype=torch.float64)
    wt = torch.tensor(rng.standard_normal((1, 3, 3, 1, 32)) / 3, dtype=torch.float64, requires_grad=True)
    y_ref = tf_ops.conv_nd_same(x, wt)
    dy = rng.standard_normal(tuple(y_ref.shape))
    y_ref.backward(torch.tensor(dy))
    d = ops.conv3d_desc(x.shape, 32, 1, (1, 1, 1))
    y, stats, rows = ops.conv3d_fwd(dev(x.numpy()), dev(wt.detach().numpy()), d, want_stats=True)
    assert rel_err(y.cpu().numpy(), y_ref.detach().numpy()) < 3e-6
    dw = ops.conv3d_wgrad(dev(x.numpy()), dev(dy), d)
    assert rel_err(dw.cpu().numpy(), wt.grad.numpy()) < 5e-6
