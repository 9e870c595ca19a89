"""UNet3D --compute_dtype bf16c (UNETK_BF16 for the stride-1 3-D convs, include/unetk.h): the new entry points
unetk_conv3d_{fwd,dgrad,wgrad}_bf16 against float64 on bf16-rounded operands, their refusals, the whole net against the
float64 oracle of the same arithmetic, and training next to the fp32 mode."""
import argparse
import math

import numpy as np
import pytest
import torch

from oracle import tf_ops, unet3d

pytestmark = pytest.mark.gpu

_conv_nd_same = tf_ops.conv_nd_same            # the oracle's own conv, captured before any test wraps it
_conv_transpose_ks = tf_ops.conv_transpose_ks


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    return _ops


def r16(t):
    return tf_ops.bf16_round(t)


# ----------------------------------------------------------------------------- op level
CASES = [
    # N, D, H, W, Cin, Cout, kd, extra pixel stride of x (0 = dense)
    (1, 2, 96, 96, 32, 32, 1, 0),          # conv_e0/conv2, conv_d0/conv2 at 96^2
    (1, 2, 48, 48, 64, 64, 1, 0),          # conv_e1/conv2 at 48^2
    (1, 3, 24, 24, 128, 128, 3, 0),        # conv_e2/conv2 at 24^2
    (1, 3, 12, 12, 256, 256, 3, 0),        # conv_e3/conv2 at 12^2
    (1, 3, 6, 6, 320, 320, 3, 0),          # bridge/conv2 at 6^2
    (1, 2, 12, 12, 512, 256, 3, 64),       # conv_d3/conv1: a 512-channel concat input read through a pixel stride
    (2, 2, 24, 24, 128, 64, 3, 0),         # batch 2, D = 2: both depth edges of every plane read the zero page
]


def _ref(x, w, dy):
    """float64 on bf16-rounded operands (and the magnitudes sum |a b| the accumulation-order noise scales with)."""
    xr, wr = r16(x).requires_grad_(True), r16(w).requires_grad_(True)
    y = _conv_nd_same(xr, wr)
    dx, dw = torch.autograd.grad(y, (xr, wr), r16(dy))
    xa, wa = xr.detach().abs().requires_grad_(True), wr.detach().abs().requires_grad_(True)
    ya = _conv_nd_same(xa, wa)
    dxa, dwa = torch.autograd.grad(ya, (xa, wa), r16(dy).abs())
    return y.detach(), dx, dw, ya.detach(), dxa, dwa


def _err(got, ref, mag):
    return ((got.double() - ref).abs() / mag.clamp_min(1e-30)).max().item()


@pytest.mark.parametrize("case", CASES)
def test_conv3d_bf16_against_float64_on_rounded_operands(ops, case):
    from boxsegliver_amd import _abi
    n, dd, h, w, cin, cout, kd, extra = case
    g = torch.Generator(device="cuda").manual_seed(cin * 31 + cout + h + n)
    xs = cin + extra
    xbuf = torch.randn((n, dd, h, w, xs), generator=g, device="cuda", dtype=torch.float32)
    x = xbuf[..., :cin]
    wt = (torch.randn((kd, 3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * kd * cin)).contiguous()
    dy = torch.randn((n, dd, h, w, cout), generator=g, device="cuda")
    y_ref, dx_ref, dw_ref, y_mag, dx_mag, dw_mag = _ref(x.double(), wt.double(), dy.double())

    d = ops.conv3d_desc(x.shape, cout, kd, (1, 1, 1), x_stride=xs)
    assert ops.conv3d_bf16_ok(d)
    wp_f, wp_d = ops.conv3d_pack(wt, precision=_abi.BF16)
    assert wp_f.dtype == torch.bfloat16 and wp_f.numel() == kd * 9 * cin * cout
    y, stats, rows = ops.conv3d_fwd(x, wp_f, d, want_stats=True, precision=_abi.BF16)
    dense = ops.conv3d_desc((n, dd, h, w, cin), cout, kd, (1, 1, 1))
    dx = ops.conv3d_dgrad(dy, wp_d, dense, precision=_abi.BF16)
    dw = ops.conv3d_wgrad(x, dy, d, precision=_abi.BF16)
    torch.cuda.synchronize()
    ey, edx, edw = _err(y, y_ref, y_mag), _err(dx, dx_ref, dx_mag), _err(dw, dw_ref, dw_mag)
    print(case, "y", ey, "dx", edx, "dw", edw)
    assert ey < 2e-5 and edx < 2e-5 and edw < 2e-5

    # statistic partials: each sample's rows contiguous, fp32 sums of the fp32 accumulators
    assert rows % n == 0
    per = stats.double().reshape(2, n, rows // n, cout).sum(2)
    yd = y.double()
    s1, s2 = yd.sum((1, 2, 3)), (yd * yd).sum((1, 2, 3))
    assert ((per[0] - s1).abs() / yd.abs().sum((1, 2, 3)).clamp_min(1e-30)).max().item() < 1e-5
    assert ((per[1] - s2).abs() / s2.clamp_min(1e-30)).max().item() < 1e-5

    # the bf16 pipe really ran: the exact-fp32 path differs by the operand rounding, far above accumulation noise
    wp32_f, wp32_d = ops.conv3d_pack(wt)
    y32, _, _ = ops.conv3d_fwd(x, wp32_f, d, want_stats=False)
    dx32 = ops.conv3d_dgrad(dy, wp32_d, dense)
    dw32 = ops.conv3d_wgrad(x, dy, d)
    for got, exact, mag, e in ((y, y32, y_mag, ey), (dx, dx32, dx_mag, edx), (dw, dw32, dw_mag, edw)):
        diff = _err(got, exact.double(), mag)
        assert diff > 3e-5 and diff > 5 * e, (diff, e)

    # dW is bit-reproducible run to run and identical on the side stream (ops.SIDE_WGRAD3D_VOXELS)
    dw_again = ops.conv3d_wgrad(x, dy, d, precision=_abi.BF16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dw_side = ops.conv3d_wgrad(x, dy, d, ws_pool=ops._Workspace(), precision=_abi.BF16)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw_again) and torch.equal(dw, dw_side)


def test_conv3d_bf16_refusals_on_the_device(ops):
    import ctypes
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    x = torch.zeros((1, 2, 8, 16, 64), device="cuda")
    wt = torch.zeros((3, 3, 3, 64, 64), device="cuda")
    wp_f, _ = ops.conv3d_pack(wt, precision=_abi.BF16)
    y = torch.zeros((1, 2, 8, 16, 64), device="cuda")
    d = ops.conv3d_desc(x.shape, 64, 3, (1, 1, 1))
    nb = lib.unetk_conv3d_ws_bytes_bf16(ctypes.byref(d))
    ws = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    st = _abi.stream_ptr()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    assert lib.unetk_conv3d_fwd_bf16(ctypes.byref(d), P(x), P(wp_f), P(y), None, None, nb, st) == -1
    assert lib.unetk_conv3d_fwd_bf16(ctypes.byref(d), P(x), P(wp_f), P(y), None, P(ws, 4), nb, st) == -1
    assert lib.unetk_conv3d_fwd_bf16(ctypes.byref(d), P(x), P(wp_f), P(y), None, P(ws), nb - 16, st) == -3
    assert lib.unetk_conv3d_wgrad_bf16(ctypes.byref(d), P(x), P(y), P(wt), P(ws), nb - 16, st) == -3
    s2 = ops.conv3d_desc(x.shape, 64, 3, (1, 2, 2))
    assert lib.unetk_conv3d_fwd_bf16(ctypes.byref(s2), P(x), P(wp_f), P(y), None, P(ws), nb, st) == -2
    with pytest.raises(_abi.UnetkError):
        ops.conv3d_fwd(x, wp_f, s2, precision=_abi.BF16)
    assert ops.conv3d_precision(s2, _abi.BF16) == _abi.FP32 and ops.conv3d_precision(d, _abi.BF16) == _abi.BF16
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- whole net
YML = dict(init_channels=30, max_channels=320, num_pool_layers=4, ret_prob=False, ret_pred=True, build_metrics=True,
           build_summaries=False)


def make_args(**over):
    a = argparse.Namespace(
        classes=["NF"], batch_size=2, num_gpus=1, im_depth=8, im_height=64, im_width=64, im_channel=1,
        normalizer="instance_norm", without_norm=False, weight_init="xavier", weight_decay_rate=3e-5, bias_decay=False,
        loss_type="xentropy", loss_weight_type="numerical", loss_numeric_w=[1.0, 1.0], loss_proportion_decay=1000,
        metrics_train=["Dice"], img_grad=False, tag="test3d_bf16c", seed=1234, use_spatial=False, guide_channel=2,
        learning_rate=3e-4, learning_policy="period_step", lr_decay_step=100000, lr_decay_rate=0.1,
        num_of_total_steps=1000, lr_power=0.9, lr_end=1e-6, lr_decay_boundaries=None, lr_custom_values=None,
        optimizer="Adam", eval_per_epoch=False, compute_dtype="bf16c")
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _params(net):
    params = unet3d.init_params(net.specs, seed=5)
    g = torch.Generator().manual_seed(9)
    for name, _, kind in net.specs:
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(params[name].shape, generator=g)
        elif kind in ("beta", "bias"):
            params[name] = 0.1 * torch.randn(params[name].shape, generator=g)
    return params


def _build(args):
    from boxsegliver_amd.NetworksV2.UNet3D import UNet3D
    from boxsegliver_amd.data.synthetic import make_batch_3d
    images, labels, _ = make_batch_3d(2, args.im_depth, args.im_height, args.im_width, 1, 2, 1234)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda()}
    model = UNet3D(args)
    model(inputs, "eval", **YML)
    return model, inputs


class _Bf16Operands(torch.autograd.Function):
    """UNETK_BF16 arithmetic of one stride-1 conv: y = conv(r(x), r(w)); dx = conv^T(r(dy), r(w)); dw = corr(r(x), r(dy))."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _conv_nd_same(r16(x), r16(w))

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            xr, wr = r16(x).requires_grad_(True), r16(w).requires_grad_(True)
            dx, dw = torch.autograd.grad(_conv_nd_same(xr, wr), (xr, wr), r16(dy))
        return dx, dw


class _Bf16OperandsT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride):
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return _conv_transpose_ks(r16(x), r16(w), stride)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            xr, wr = r16(x).requires_grad_(True), r16(w).requires_grad_(True)
            dx, dw = torch.autograd.grad(_conv_transpose_ks(xr, wr, ctx.stride), (xr, wr), r16(dy))
        return dx, dw, None


def bf16c_conv(x, w, stride=None, bias=None, dilation=1):
    """The layer rule in the oracle's logical (un-padded) channels: stride 1 and a padded channel count on both sides
    (every conv but the first, whose Cin = 1 image is not padded); kd is 1 or 3 everywhere in UNet3D."""
    assert bias is None and dilation == 1
    if (stride is None or all(s == 1 for s in stride)) and w.shape[-2] >= 16 and w.shape[0] in (1, 3):
        return _Bf16Operands.apply(x, w)
    return _conv_nd_same(x, w, stride=stride)


def bf16c_conv_transpose(x, w, stride, bias=None):
    assert bias is None
    return _Bf16OperandsT.apply(x, w, tuple(stride))


def _grad_l2(model, grads):
    num = den = 0.0
    for name in model.params.trainable_names():
        d = model.params.logical_grad(name).cuda().double() - grads[name]
        num += float((d * d).sum())
        den += float((grads[name] * grads[name]).sum())
    return (num / den) ** 0.5


@pytest.mark.parametrize("normalizer", ["instance_norm", "batch_norm"])
def test_unet3d_bf16c_against_device_float64_oracle_of_the_same_arithmetic(monkeypatch, normalizer):
    args = make_args(normalizer=normalizer)
    model, inputs = _build(args)
    net = unet3d.UNet3DOracle(1, 2, normalizer=normalizer)
    params = _params(net)
    model.params.load_state(params)
    monkeypatch.setattr(tf_ops, "conv_nd_same", bf16c_conv)
    monkeypatch.setattr(tf_ops, "conv_transpose_ks", bf16c_conv_transpose)
    p64 = {k: v.double().cuda() for k, v in params.items()}
    total, _, logits, grads, _ = net.loss_and_grads(
        p64, inputs["images"].double(), inputs["labels"].long(), loss_type=args.loss_type,
        loss_weight_type=args.loss_weight_type, numeric_w=args.loss_numeric_w, weight_decay_rate=args.weight_decay_rate)
    model.params.zero_grad()
    loss = model(inputs, "train", **YML)
    loss.backward()
    torch.cuda.synchronize()
    got = model.layers["logits"].double()
    d = (got - logits).abs()
    agree = (got.argmax(-1) == logits.argmax(-1)).double().mean().item()
    gl2 = _grad_l2(model, grads)
    print(normalizer, "loss", abs(loss.item() - total.item()), "logits max", d.max().item(), "mean", d.mean().item(),
          "argmax", agree, "gradL2", gl2)
    assert abs(loss.item() - total.item()) < 1e-3 * max(1.0, abs(total.item()))
    assert d.max().item() < 5e-2 and d.mean().item() < 5e-3
    assert agree > 0.995
    assert gl2 < 0.1


def test_unet3d_bf16_storage_still_refused_and_names_bf16c():
    args = make_args(compute_dtype="bf16", im_depth=4, im_height=32, im_width=32)
    with pytest.raises(NotImplementedError, match="bf16c"):
        _build(args)


def test_unet3d_bf16c_trains_beside_fp32_and_keeps_the_padding_zero():
    """Ten Adam steps of fp32 and of bf16c from the same weights and batch; the bf16c model starts from the fp32 model's
    state_dict (checkpoints are fp32 master weights in either mode)."""
    from boxsegliver_amd.core.solver import Solver
    curves = {}
    state = None
    for mode in ("fp32", "bf16c"):
        args = make_args(compute_dtype=mode, im_depth=4, im_height=32, im_width=32)
        model, inputs = _build(args)
        if state is None:
            net = unet3d.UNet3DOracle(1, 2, normalizer=args.normalizer)
            model.params.load_state(_params(net))
            state = {k: v.clone() for k, v in model.params.state_dict().items()}
        else:
            model.params.load_state(state)
        solver = Solver(args)
        losses = []
        for _ in range(10):
            loss = model(inputs, "train", **YML)
            losses.append(loss.item())
            solver(loss, model)
        curves[mode] = np.array(losses)
        w = model.params["UNet3D/conv_d0/conv1/weights"].detach()
        assert float(w[..., 30:32, :].abs().sum()) == 0.0 and float(w[..., 62:64, :].abs().sum()) == 0.0
        assert float(w[..., 30:32].abs().sum()) == 0.0
        w = model.params["UNet3D/conv_e3/conv2/weights"].detach()
        assert float(w[..., 240:, :].abs().sum()) == 0.0 and float(w[..., 240:].abs().sum()) == 0.0
        model(inputs, "eval", **YML)
        assert model.predictions["NFPred"].dtype == torch.uint8
    print("fp32", curves["fp32"], "bf16c", curves["bf16c"])
    assert curves["fp32"][-1] < curves["fp32"][0]
    np.testing.assert_allclose(curves["bf16c"], curves["fp32"], rtol=3e-2)
