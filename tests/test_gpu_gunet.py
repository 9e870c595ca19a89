"""GPU parity of the GUNet plugin (spatial-guide path, BASELINE.json configs[3] at reduced size) against
the CPU oracle: logits / loss / gradients / moving statistics, every conv unit's backward on identical
operands (instance norm + centre-only + guide modulation, and the batch-norm variant), xentropy+dice."""
import argparse

import numpy as np
import pytest
import torch

from oracle import gunet2d
from test_gpu_unet import check_deconv_backward, check_unit_backward, rel
from unetk_rng import fc_uniform_host, unit_mask_host          # shared with test_gpu_norm_paths.py

pytestmark = pytest.mark.gpu

YML = dict(init_channels=64, num_down_samples=4, mod_layers=[1, 2, 3, 4], context_fc_channels=[256, 256],
           context_model="fc", context_conv_init_channels=2, norm_with_center=True, norm_with_scale=False,
           ret_prob=False, ret_pred=True, build_metrics=True, build_summaries=False)


def make_args(**over):
    a = argparse.Namespace(
        classes=["Liver", "Tumor"], batch_size=2, num_gpus=1, im_height=32, im_width=32, im_channel=3,
        normalizer="instance_norm", without_norm=False, weight_init="xavier", weight_decay_rate=1e-5, bias_decay=False,
        loss_type="xentropy", loss_weight_type="numerical", loss_numeric_w=[0.2, 0.4, 4.4], loss_proportion_decay=1000,
        metrics_train=["Dice"], img_grad=False, tag="test", seed=1234, use_spatial=True, use_context=False,
        side_dropout=0.5, dropout=None, use_se=False, fix=False, guide_channel=1,
        learning_rate=1e-3, learning_policy="period_step", lr_decay_step=100000, lr_decay_rate=0.1,
        num_of_total_steps=1000, lr_power=0.9, lr_end=1e-6, lr_decay_boundaries=None, lr_custom_values=None,
        optimizer="Adam", eval_per_epoch=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def setup(args, size=32):
    from boxsegliver_amd.NetworksV2.GUNet import GUNet
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    images, labels, _ = make_batch(2, size, size, 3, 3, 1234)
    guide = make_guide(labels, args.guide_channel, 1234)
    model = GUNet(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda()}
    model(inputs, "eval", **YML)
    net = gunet2d.GUNet2DOracle(3, 3, guide_channel=args.guide_channel, normalizer=args.normalizer,
                                without_norm=bool(getattr(args, "without_norm", False)))
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.specs]
    gen = torch.Generator().manual_seed(11)
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        elif "spatial" in name:
            params[name] = 0.5 * torch.randn(t.shape, generator=gen)
        else:
            params[name] = t.clone()
    model.params.load_state(params)
    return model, inputs, net, params, (torch.from_numpy(images), torch.from_numpy(guide), torch.from_numpy(labels).long())


def kwargs_of(args):
    return dict(loss_type=args.loss_type, loss_weight_type=args.loss_weight_type, numeric_w=args.loss_numeric_w,
                proportion_decay=args.loss_proportion_decay, weight_decay_rate=args.weight_decay_rate)


@pytest.mark.parametrize("normalizer,loss_type,g_ch", [("instance_norm", "xentropy", 1), ("batch_norm", "xentropy+dice", 2),
                                                       ("without_norm", "xentropy", 1)])
def test_gunet_matches_oracle(normalizer, loss_type, g_ch):
    from boxsegliver_amd import ops
    without_norm = normalizer == "without_norm"          # GUNet.py:251-252,314-315: conv + bias (+ guide) + ReLU units
    normalizer = "batch_norm" if without_norm else normalizer
    args = make_args(normalizer=normalizer, loss_type=loss_type, guide_channel=g_ch, without_norm=without_norm)
    model, inputs, net, params, (images, guide, labels) = setup(args)
    total, _, logits, grads, new_stats = net.loss_and_grads(params, images, guide, labels, **kwargs_of(args))
    p64 = {k: v.double() for k, v in params.items()}
    _, _, _, grads64, _ = net.loss_and_grads(p64, images.double(), guide.double(), labels, **kwargs_of(args))
    ops.DEBUG_CAPTURE = []
    try:
        model.params.zero_grad()
        loss = model(inputs, "train", **YML)
        loss.backward()
        torch.cuda.synchronize()
        captured = ops.DEBUG_CAPTURE
    finally:
        ops.DEBUG_CAPTURE = None
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    got = model.layers["logits"].cpu().numpy()
    assert np.abs(got - logits.numpy()).max() < 1e-3
    srt = np.sort(logits.numpy(), -1)
    safe = (srt[..., -1] - srt[..., -2]) > 1e-3
    assert (got.argmax(-1) == logits.numpy().argmax(-1))[safe].all()
    # every backward kernel on identical operands (18 units: 8 modulated, centre-only)
    units = [c for c in captured if c.get("kind") != "deconv"]
    assert len(units) == 18 and len(captured) == 22
    assert sum(1 for c in units if c["gw"] is not None) == 8
    assert all(bool(c.get("plain")) == without_norm for c in units)
    assert ("GUNet/Encode/down_conv2/mod_conv1/biases" in model.params.state_dict()) == without_norm
    for c in units:
        check_unit_backward(c)
    for c in captured:
        if c.get("kind") == "deconv":
            check_deconv_backward(c)
    # end-to-end gradients in L2 (mask flips, see test_gpu_unet.py)
    num = den = 0.0
    for name in model.params.trainable_names():
        g = model.params[name].grad.cpu().numpy().astype(np.float64)
        if model.params.where[name][0] == "reg":
            # the L2 term's gradient (wd * w) is applied inside the optimiser kernel (Solver.apply_gradients), not by
            # backward(); the oracle differentiates data loss + regulariser.  Without normalisation the deep levels' data
            # gradients are as small as this term, so it must be accounted for
            g = g + args.weight_decay_rate * model.params[name].detach().cpu().numpy().astype(np.float64)
        ref = grads64[name].numpy()
        l2 = np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30)
        assert l2 < 1e-1, (name, l2)            # tiny tensors fed by 4..32 pixels feel single mask flips
        num += np.sum((g - ref) ** 2)
        den += np.sum(ref ** 2)
    # whole gradient vector.  At 32 x 32 the bridge normalises over 2 x 2 = FOUR values per (sample, channel): one ReLU mask
    # that flips there (a pre-activation within rounding of 0) moves the whole vector by 0.6-4 %, and whether one flips is a
    # matter of the last bit of the statistics.  Measured over six parameter draws of this very test (logits within 1.2e-5 of
    # float64 in every one): device 1.1e-5, 1.8e-5, 6.6e-3, 7.2e-3, 3.1e-2, 4.0e-2; the fp32 CPU oracle 9e-6 .. 4e-3 -- a
    # discrete distribution, not an error level.  The kernels are pinned on identical operands above (1e-5); this bar only
    # says that nothing systematic is off.
    assert (num / den) ** 0.5 < 6e-2
    for name, ref in new_stats.items():
        np.testing.assert_allclose(model.params[name].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)
    assert model.name == "GUNet" and model.metrics_dict["Liver/Dice"].item() >= 0.0


def test_gunet_trains_and_checkpoint_names():
    from boxsegliver_amd.core.solver import Solver
    args = make_args()
    model, inputs, net, params, _ = setup(args)
    names = list(model.params.state_dict())
    assert "GUNet/spatial/conv2/weights" in names and "GUNet/Encode/down_conv2/mod_conv1/InstanceNorm/beta" in names
    assert "GUNet/Encode/down_conv2/mod_conv1/InstanceNorm/gamma" not in names          # norm_with_scale: false
    assert "GUNet/Encode/down_conv1/mod_conv1/InstanceNorm/gamma" in names              # level 0 is not modulated
    assert "GUNet/Decode/up_conv1/up_conv1_2/InstanceNorm/gamma" in names
    solver = Solver(args)
    first = None
    for _ in range(4):
        loss = model(inputs, "train", **YML)
        first = loss.item() if first is None else first
        solver(loss, model)
    assert model(inputs, "train", **YML).item() < first
    model(inputs, "eval", **YML)
    assert model.probability.shape == (2, 32, 32, 3)


# ----------------------------------------------------------------------------- context (density) branch, GUNet.py:31-60


@pytest.mark.parametrize("bsz,k,n,relu,keep", [(2, 10, 256, True, None), (8, 256, 1000, True, 0.5), (3, 256, 3968, False, None),
                                               (5, 33, 70, True, 0.8)])
def test_fully_connected_forward_backward_and_dropout_mask(bsz, k, n, relu, keep):
    from boxsegliver_amd import ops
    gen = torch.Generator().manual_seed(bsz * 1000 + n)
    x = torch.randn(bsz, k, generator=gen)
    w = torch.randn(k, n, generator=gen) / k ** 0.5
    b = torch.randn(n, generator=gen)
    dy = torch.randn(bsz, n, generator=gen)
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    seed = 77
    y = ops.FullyConnected.apply(xd, wd, bd, relu, keep, seed)
    y.backward(dy.cuda())
    mask = None
    if keep is not None:
        u = fc_uniform_host(seed, np.arange(bsz * n, dtype=np.uint64)).reshape(bsz, n)
        mask = torch.from_numpy(np.where(u < np.float32(keep), np.float32(1.0) / np.float32(keep), np.float32(0)))
        assert abs((mask > 0).float().mean().item() - keep) < 0.05
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = x64 @ w64 + b64
    if relu:
        ref = torch.relu(ref)
    if mask is not None:
        ref = ref * mask.double()
    ref.backward(dy.double())
    assert rel(y.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    if mask is not None:                                   # the mask itself: dropped entries are exact zeros
        np.testing.assert_array_equal(y.detach().cpu().numpy()[mask.numpy() == 0], 0.0)
    assert rel(xd.grad.cpu().numpy(), x64.grad.numpy()) < 1e-5
    assert rel(wd.grad.cpu().numpy(), w64.grad.numpy()) < 1e-5
    assert rel(bd.grad.cpu().numpy(), b64.grad.numpy()) < 1e-5
    # bit-reproducible
    xd2, wd2, bd2 = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y2 = ops.FullyConnected.apply(xd2, wd2, bd2, relu, keep, seed)
    y2.backward(dy.cuda())
    assert torch.equal(y, y2) and torch.equal(wd.grad, wd2.grad) and torch.equal(xd.grad, xd2.grad)


@pytest.mark.parametrize("per_sample,g_ch,n,hw,c", [(True, 0, 3, 24 * 24, 64), (False, 0, 4, 16 * 16, 128), (False, 2, 2, 32 * 32, 64),
                                                    (True, 1, 2, 8 * 8, 512), (False, 0, 32, 16 * 16, 1024)])
def test_norm_density_modulation_forward_backward(per_sample, g_ch, n, hw, c):
    """z = relu(norm(y) * den[b, c] [+ guide . gw + gb]) and its backward (dy, dgamma, dbeta, dden, dgw, dgb) against
    float64 autograd on the same operands -- the kernels of csrc/norm.hip with the D flag."""
    from boxsegliver_amd import ops
    from oracle import tf_ops
    gen = torch.Generator().manual_seed(c + n)
    h = int(hw ** 0.5)
    y = torch.randn(n, h, h, c, generator=gen) * 2 + 0.5
    gamma = 0.5 + torch.rand(c, generator=gen)
    beta = 0.3 * torch.randn(c, generator=gen)
    den = 1.0 + 0.5 * torch.randn(n, c, generator=gen)       # signs included
    dz = torch.randn(n, h, h, c, generator=gen)
    guide = torch.rand(n, h, h, g_ch, generator=gen) if g_ch else None
    gw = torch.randn(g_ch, c, generator=gen) if g_ch else None
    gb = 0.1 * torch.randn(c, generator=gen) if g_ch else None
    yd = y.cuda()
    d = ops.norm_desc(y.shape, per_sample, c, g_ch, c if g_ch else 0, 0)
    # statistics partials: one row per sample (sum, sum of squares)
    flat = yd.reshape(n, hw, c)
    stats = torch.stack([flat.sum(1), (flat * flat).sum(1)]).contiguous()
    aff = ops.norm_finalize(d, stats, n, gamma.cuda(), beta.cuda(), 1e-3 if not per_sample else 1e-6, 0.99, True,
                            torch.zeros(c).cuda(), torch.ones(c).cuda(), yd.device)
    cu = lambda t: None if t is None else t.cuda().contiguous()
    z = torch.empty_like(yd)
    ops.norm_apply_relu(d, yd, aff, z, cu(guide), cu(gw), cu(gb), cu(den))
    dy, dgamma, dbeta, dgw, dgb, dden = ops.norm_relu_bwd(d, yd, cu(dz), aff, True, True, cu(guide), cu(gw), cu(gb), cu(den))
    d64 = lambda t: None if t is None else t.double().requires_grad_(True)
    y64, g64, b64, den64, gw64, gb64 = d64(y), d64(gamma), d64(beta), d64(den), d64(gw), d64(gb)
    if per_sample:
        t = tf_ops.instance_norm(y64, g64, b64, eps=1e-6)
    else:
        t, _, _ = tf_ops.batch_norm(y64, g64, b64, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64), True)
    u = t * den64[:, None, None, :]
    if g_ch:
        u = u + (guide.double() @ gw64 + gb64)
    ref = torch.relu(u)
    ref.backward(dz.double())
    tol = 2e-5
    assert rel(z.cpu().numpy(), ref.detach().numpy()) < tol
    assert rel(dy.cpu().numpy(), y64.grad.numpy()) < tol
    assert rel(dgamma.cpu().numpy(), g64.grad.numpy()) < tol
    assert rel(dbeta.cpu().numpy(), b64.grad.numpy()) < tol
    assert rel(dden.cpu().numpy(), den64.grad.numpy()) < tol
    if g_ch:
        assert rel(dgw.cpu().numpy(), gw64.grad.numpy()) < tol
        assert rel(dgb.cpu().numpy(), gb64.grad.numpy()) < tol
    # reproducible, and den = 1 reduces bit-exactly to the un-modulated kernels
    again = ops.norm_relu_bwd(d, yd, cu(dz), aff, True, True, cu(guide), cu(gw), cu(gb), cu(den))
    assert all(torch.equal(a, b) for a, b in zip((dy, dgamma, dbeta, dden), (again[0], again[1], again[2], again[5])))
    ones = torch.ones(n, c).cuda()
    z1, z0 = torch.empty_like(yd), torch.empty_like(yd)
    ops.norm_apply_relu(d, yd, aff, z1, cu(guide), cu(gw), cu(gb), ones)
    ops.norm_apply_relu(d, yd, aff, z0, cu(guide), cu(gw), cu(gb))
    assert torch.equal(z1, z0)


def setup_context(args, size=32, bsz=2, ctx_len=10, use_spatial=True):
    from boxsegliver_amd.NetworksV2.GUNet import GUNet
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    images, labels, _ = make_batch(bsz, size, size, 3, 3, 1234)
    guide = make_guide(labels, args.guide_channel, 1234)
    gen = torch.Generator().manual_seed(5)
    context = torch.rand(bsz, ctx_len, generator=gen)
    model = GUNet(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda(), "context": context.cuda()}
    model(inputs, "eval", **YML)
    net = gunet2d.GUNet2DOracle(3, 3, guide_channel=args.guide_channel, normalizer=args.normalizer, use_spatial=use_spatial,
                                context_length=ctx_len, context_fc_channels=YML["context_fc_channels"])
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.specs]
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias", "fc_b"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        elif "spatial" in name:
            params[name] = 0.5 * torch.randn(t.shape, generator=gen)
        else:
            params[name] = t.clone()
    last = "GUNet/context/fc3/biases"
    params[last] = params[last] + 1.0                          # gains around 1 (he_normal weights, unit offset)
    model.params.load_state(params)
    return model, inputs, net, params, (torch.from_numpy(images), torch.from_numpy(guide), torch.from_numpy(labels).long(),
                                        context)


@pytest.mark.parametrize("normalizer,use_spatial,side_dropout", [("instance_norm", True, 0.0), ("batch_norm", False, 0.0),
                                                                 ("instance_norm", True, 0.5)])
def test_gunet_context_branch_matches_oracle(normalizer, use_spatial, side_dropout):
    """--use_context: the MLP's gains modulate every encoder unit of the mod_layers (GUNet.py:203-206).  With dropout
    the oracle is fed the masks the device drew (read back from the autograd nodes), so the arithmetic is compared."""
    from boxsegliver_amd import ops
    args = make_args(normalizer=normalizer, use_context=True, use_spatial=use_spatial, side_dropout=side_dropout)
    model, inputs, net, params, (images, guide, labels, context) = setup_context(args, use_spatial=use_spatial)
    names = list(model.params.state_dict())
    assert "GUNet/context/fc1/weights" in names and "GUNet/context/fc3/biases" in names
    assert model.params["GUNet/context/fc3/weights"].shape == (256, 64 * (2 + 4 + 8 + 16) * 2)
    assert ("GUNet/spatial/conv2/weights" in names) == use_spatial
    ops.DEBUG_CAPTURE = []
    try:
        model.params.zero_grad()
        loss = model(inputs, "train", **YML)
        masks = None
        if side_dropout:
            # walk the autograd graph of the context params for the two dropout masks (fc1, fc2 order)
            fn, found = model.layers["context_params"].grad_fn, []
            while fn is not None and type(fn).__name__ == "FullyConnectedBackward":
                found.append(fn.saved_tensors[3])
                fn = fn.next_functions[0][0]
            masks = [m.cpu() for m in reversed(found) if m is not None]
            assert len(masks) == 2 and all(0.3 < (m > 0).float().mean().item() < 0.7 for m in masks)
            assert all(set(np.unique(m.numpy()).tolist()) <= {0.0, 2.0} for m in masks)
        loss.backward()
        torch.cuda.synchronize()
        captured = ops.DEBUG_CAPTURE
    finally:
        ops.DEBUG_CAPTURE = None
    kw = dict(kwargs_of(args), context=context, drop_masks=masks)
    total, _, logits, grads, new_stats = net.loss_and_grads(params, images, guide, labels, **kw)
    p64 = {k: v.double() for k, v in params.items()}
    kw64 = dict(kw, context=context.double(), drop_masks=None if masks is None else [m.double() for m in masks])
    _, _, _, grads64, _ = net.loss_and_grads(p64, images.double(), guide.double(), labels, **kw64)
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    assert np.abs(model.layers["logits"].cpu().numpy() - logits.numpy()).max() < 1e-3
    den_ref = net.context_params(p64, context.double(), kw64["drop_masks"]).numpy()
    assert rel(model.layers["context_params"].detach().cpu().numpy(), den_ref) < 1e-5
    units = [c for c in captured if c.get("kind") != "deconv"]
    assert sum(1 for c in units if c.get("den") is not None) == 8
    for c in units:
        check_unit_backward(c)
    num = den = 0.0
    for name in model.params.trainable_names():
        g = model.params[name].grad.cpu().numpy().astype(np.float64)
        ref = grads64[name].numpy()
        l2 = np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30)
        # (the 2x2-pixel level's tensors feel single ReLU flips; the kernels are pinned on identical operands above)
        assert l2 < (2e-1 if ("conv5" in name or "down_conv5" in name) else 1e-1), (name, l2)
        num += np.sum((g - ref) ** 2)
        den += np.sum(ref ** 2)
    assert (num / den) ** 0.5 < 5e-3
    for name in ("GUNet/context/fc1/weights", "GUNet/context/fc2/weights", "GUNet/context/fc3/weights",
                 "GUNet/context/fc3/biases"):
        g = model.params[name].grad.cpu().numpy()
        assert np.abs(g).max() > 0 and rel(g, grads64[name].numpy()) < 2e-2, name
    for name, ref in new_stats.items():
        np.testing.assert_allclose(model.params[name].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)


def test_gunet_context_trains_eval_has_no_dropout_and_masks_change_per_step():
    from boxsegliver_amd.core.solver import Solver
    args = make_args(use_context=True, side_dropout=0.5)
    model, inputs, net, params, (images, guide, labels, context) = setup_context(args)
    # eval: no dropout -> equals the oracle without masks, and is deterministic
    model(inputs, "eval", **YML)
    lg, _ = net.forward(params, images, guide, False, context, None)
    assert np.abs(model.layers["logits"].cpu().numpy() - lg.numpy()).max() < 1e-3
    a = model.layers["context_params"].clone()
    model(inputs, "eval", **YML)
    assert torch.equal(a, model.layers["context_params"])
    # train: a fresh mask every call
    model(inputs, "train", **YML)
    t1 = model.layers["context_params"].detach().clone()
    model(inputs, "train", **YML)
    assert not torch.equal(t1, model.layers["context_params"].detach())
    solver = Solver(args)
    losses = []
    for _ in range(6):
        loss = model(inputs, "train", **YML)
        losses.append(loss.item())
        solver(loss, model)
    assert min(losses[3:]) < losses[0]
    # FC variables are not L2-regularised (slim.fully_connected has no regulariser in _net_arg_scope, GUNet.py:244-248)
    assert model.params.where["GUNet/context/fc1/weights"][0] == "noreg"


# ----------------------------------------------------------------------------- after_affine (GUNetV2.yml, *_AA.yml)
@pytest.mark.parametrize("per_sample,with_den", [(True, True), (False, True), (False, False)])
def test_norm_post_shift_without_guide(per_sample, with_den):
    """gb with guide_ch == 0: z = relu(norm(y) [* den] + gb) -- the kernel form of after_affine (csrc/norm.hip)."""
    from boxsegliver_amd import ops
    from oracle import tf_ops
    n, h, c = 3, 16, 128
    gen = torch.Generator().manual_seed(3)
    y = torch.randn(n, h, h, c, generator=gen) + 0.3
    den = (1.0 + 0.5 * torch.randn(n, c, generator=gen)) if with_den else None
    gb = 0.3 * torch.randn(c, generator=gen)
    dz = torch.randn(n, h, h, c, generator=gen)
    yd = y.cuda()
    d = ops.norm_desc(y.shape, per_sample, c)
    flat = yd.reshape(n, h * h, c)
    stats = torch.stack([flat.sum(1), (flat * flat).sum(1)]).contiguous()
    aff = ops.norm_finalize(d, stats, n, None, None, 1e-6 if per_sample else 1e-3, 0.99, True, torch.zeros(c).cuda(),
                            torch.ones(c).cuda(), yd.device)
    cu = lambda t: None if t is None else t.cuda().contiguous()
    z = torch.empty_like(yd)
    ops.norm_apply_relu(d, yd, aff, z, None, None, cu(gb), cu(den))
    out = ops.norm_relu_bwd(d, yd, cu(dz), aff, False, False, None, None, cu(gb), cu(den))
    y64, gb64 = y.double().requires_grad_(True), gb.double().requires_grad_(True)
    den64 = den.double().requires_grad_(True) if with_den else None
    if per_sample:
        t = tf_ops.instance_norm(y64, None, None, eps=1e-6)
    else:
        t, _, _ = tf_ops.batch_norm(y64, None, None, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64), True)
    u = (t * den64[:, None, None, :] if with_den else t) + gb64
    ref = torch.relu(u)
    ref.backward(dz.double())
    assert rel(z.cpu().numpy(), ref.detach().numpy()) < 2e-5
    assert rel(out[0].cpu().numpy(), y64.grad.numpy()) < 2e-5
    assert out[3] is None and rel(out[4].cpu().numpy(), gb64.grad.numpy()) < 2e-5
    if with_den:
        assert rel(out[5].cpu().numpy(), den64.grad.numpy()) < 2e-5


@pytest.mark.parametrize("normalizer,use_spatial,use_context", [("instance_norm", True, True), ("batch_norm", True, False),
                                                               ("instance_norm", False, True)])
def test_gunet_after_affine_matches_oracle(normalizer, use_spatial, use_context):
    """ext_config/GUNetV2.yml: norm without centre / scale on the modulated levels, channel-wise affine after the
    modulation of every encoder unit (GUNet.py:213-214, 317-320)."""
    import yaml
    from pathlib import Path
    from boxsegliver_amd import ops
    from boxsegliver_amd.NetworksV2.GUNet import GUNet
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    cfg = yaml.safe_load((Path(ops.__file__).parent / "NetworksV2" / "ext_config" / "GUNetV2.yml").read_text())
    assert cfg["after_affine"] is True and cfg["context_fc_channels"] == [200, 200]
    yml = dict(cfg, build_metrics=True, build_summaries=False)
    args = make_args(normalizer=normalizer, use_spatial=use_spatial, use_context=use_context, side_dropout=0.0)
    images, labels, _ = make_batch(2, 32, 32, 3, 3, 1234)
    guide = make_guide(labels, args.guide_channel, 1234)
    gen = torch.Generator().manual_seed(9)
    context = torch.rand(2, 12, generator=gen)
    model = GUNet(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda(), "context": context.cuda()}
    model(inputs, "eval", **yml)
    net = gunet2d.GUNet2DOracle(3, 3, guide_channel=1, normalizer=normalizer, norm_with_center=False, norm_with_scale=False,
                                use_spatial=use_spatial, context_length=12 if use_context else None,
                                context_fc_channels=(200, 200), after_affine=True)
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.specs]
    names = list(model.params.state_dict())
    assert "GUNet/Encode/down_conv1/mod_conv1/ChannelWiseAffine/gamma" in names
    ns = "BatchNorm" if normalizer == "batch_norm" else "InstanceNorm"
    assert "GUNet/Encode/down_conv2/mod_conv1/{}/beta".format(ns) not in names
    assert "GUNet/Encode/down_conv1/mod_conv1/{}/beta".format(ns) in names          # level 0 keeps its own centre / scale
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias", "fc_b"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        elif "spatial" in name:
            params[name] = 0.5 * torch.randn(t.shape, generator=gen)
        else:
            params[name] = t.clone()
    if use_context:
        params["GUNet/context/fc3/biases"] = params["GUNet/context/fc3/biases"] + 1.0
    model.params.load_state(params)
    kw = dict(kwargs_of(args), context=context if use_context else None)
    total, _, logits, _, new_stats = net.loss_and_grads(params, torch.from_numpy(images), torch.from_numpy(guide),
                                                        torch.from_numpy(labels).long(), **kw)
    p64 = {k: v.double() for k, v in params.items()}
    kw64 = dict(kw, context=context.double() if use_context else None)
    _, _, _, grads64, _ = net.loss_and_grads(p64, torch.from_numpy(images).double(), torch.from_numpy(guide).double(),
                                             torch.from_numpy(labels).long(), **kw64)
    ops.DEBUG_CAPTURE = []
    try:
        model.params.zero_grad()
        loss = model(inputs, "train", **yml)
        loss.backward()
        torch.cuda.synchronize()
        captured = ops.DEBUG_CAPTURE
    finally:
        ops.DEBUG_CAPTURE = None
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    assert np.abs(model.layers["logits"].cpu().numpy() - logits.numpy()).max() < 1e-3
    # every unit's backward on identical operands: the folded gains (den * gamma'), guide weights and post-shift
    units = [c for c in captured if c.get("kind") != "deconv"]
    assert sum(1 for c in units if c.get("den") is not None) == 10          # all ten encoder units carry the affine
    assert sum(1 for c in units if c.get("gb") is not None) == 10
    for c in units:
        check_unit_backward(c)
    num = den = 0.0
    for name in model.params.trainable_names():
        g = model.params[name].grad.cpu().numpy().astype(np.float64)
        ref = grads64[name].numpy()
        l2 = np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30)
        assert l2 < (2e-1 if ("conv5" in name or "down_conv5" in name) else 1e-1), (name, l2)
        num += np.sum((g - ref) ** 2)
        den += np.sum(ref ** 2)
    # whole gradient vector; the norms over the 2x2 / 4x4 levels of this reduced-size net (instance norm with eps 1e-6 and
    # no scale of its own under after_affine; batch norm over 8 values) amplify single ReLU flips -- the kernels
    # themselves are pinned just above (to 1e-5, with the device's own ReLU masks); this end-to-end figure moves between
    # 0.6e-2 and 1.1e-2 with the summation order of the conv tiles
    assert (num / den) ** 0.5 < 3e-2
    for name in names:
        if "ChannelWiseAffine" in name and "down_conv5" not in name:      # (L2: single upstream mask flips move single entries)
            g, ref = model.params[name].grad.cpu().numpy().astype(np.float64), grads64[name].numpy()
            assert np.abs(g).max() > 0 and np.linalg.norm(g - ref) / np.linalg.norm(ref) < 1e-1, name
    for name, ref in new_stats.items():
        np.testing.assert_allclose(model.params[name].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)


# ----------------------------------------------------------------------------- UNetInter (NetworksV2/UNetInter.py)
@pytest.mark.parametrize("normalizer,mid_cat", [("batch_norm", False), ("instance_norm", False), ("batch_norm", True),
                                                ("without_norm", False)])
def test_unetinter_matches_oracle_and_trains(normalizer, mid_cat):
    without_norm = normalizer == "without_norm"
    normalizer = "batch_norm" if without_norm else normalizer
    from boxsegliver_amd.core import models
    from boxsegliver_amd.core.solver import Solver
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    zoo = {cls.__name__: cls for cls in models.MODEL_ZOO}
    assert "UNetInter" in zoo
    args = make_args(normalizer=normalizer, use_spatial=True, guide_channel=1, mid_cat=mid_cat, without_norm=without_norm,
                     use_2d=False)
    yml = dict(init_channels=64, num_down_samples=4, ret_prob=False, ret_pred=True, build_metrics=True, build_summaries=False)
    images, labels, _ = make_batch(2, 32, 32, 3, 3, 1234)
    guide = make_guide(labels, 1, 1234)
    model = zoo["UNetInter"](args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda()}
    model(inputs, "eval", **yml)
    net = gunet2d.GUNet2DOracle(3 if mid_cat else 4, 3, guide_channel=1, normalizer=normalizer, name="UNetInter",
                                concat_guide=True, encoder_decay=0.99, mid_cat=mid_cat, without_norm=without_norm)
    lspecs = getattr(model.params, "logical_specs", model.params.specs)
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in lspecs]
    assert model.name == "UNetInter"
    st = model.params.state_dict()
    assert st["UNetInter/Encode/down_conv1/mod_conv1/weights"].shape == (3, 3, 3 if mid_cat else 4, 64)
    if mid_cat:      # --mid_cat (UNetInter.py:124-129): 64 + 1 channels into Encode2, padded to 96 on the device
        assert st["UNetInter/Encode/down_conv2/mod_conv1/weights"].shape == (3, 3, 65, 128)
        assert model.params["UNetInter/Encode/down_conv2/mod_conv1/weights"].shape == (3, 3, 96, 128)
    gen = torch.Generator().manual_seed(4)
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        else:
            params[name] = t.clone()
    model.params.load_state(params)
    total, _, logits, _, new_stats = net.loss_and_grads(params, torch.from_numpy(images), torch.from_numpy(guide),
                                                        torch.from_numpy(labels).long(), **kwargs_of(args))
    p64 = {k: v.double() for k, v in params.items()}
    _, _, _, grads64, _ = net.loss_and_grads(p64, torch.from_numpy(images).double(), torch.from_numpy(guide).double(),
                                             torch.from_numpy(labels).long(), **kwargs_of(args))
    model.params.zero_grad()
    loss = model(inputs, "train", **yml)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    assert np.abs(model.layers["logits"].cpu().numpy() - logits.numpy()).max() < 1e-3
    num = den = 0.0
    for name in model.params.trainable_names():
        g = (model.params.logical_grad(name) if mid_cat else model.params[name].grad.cpu()).numpy().astype(np.float64)
        ref = grads64[name].numpy()
        num += np.sum((g - ref) ** 2)
        den += np.sum(ref ** 2)
    assert (num / den) ** 0.5 < 1e-2
    st = model.params.state_dict()
    for name, ref in new_stats.items():                     # encoder BN decay .99, decoder .999
        np.testing.assert_allclose(st[name].numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)
    solver = Solver(args)
    first = model(inputs, "train", **yml)
    f0 = first.item()
    solver(first, model)
    for _ in range(4):
        solver(model(inputs, "train", **yml), model)
    assert model(inputs, "train", **yml).item() < f0
    if mid_cat:      # the padded filter rows stay exactly zero through training
        wt = model.params["UNetInter/Encode/down_conv2/mod_conv1/weights"].detach()
        assert float(wt[:, :, 65:, :].abs().sum()) == 0.0
    # use_2d only pins the static graph shape in the reference (UNetInter.py:76-78): accepted, nothing to do
    m2d = zoo["UNetInter"](make_args(use_spatial=True, guide_channel=1, mid_cat=False, use_2d=True))
    m2d(inputs, "eval", **yml)
    assert m2d.probability.shape == (2, 32, 32, 3)


# ----------------------------------------------------------------------------- --dropout / --fix / --use_se (GUNet.py:189-201,299-304)
@pytest.mark.parametrize("per_sample,g_ch,with_den,leaky", [(True, 0, False, False), (False, 1, False, False), (True, 2, True, False),
                                                            (False, 0, True, False), (True, 1, False, True)])
def test_norm_dropout_forward_backward(per_sample, g_ch, with_den, leaky):
    """u = norm(y) * mask [* den] [+ guide . gw + gb | + lrelu(guide . gw + gb)], z = relu(u): slim.dropout on the normalised
    value (GUNet.py:189-190) inside the norm kernels, against float64 autograd with the SAME mask (regenerated on the host)."""
    from boxsegliver_amd import ops
    from oracle import tf_ops
    n, h, c, keep, seed = 3, 12, 64, 0.7, 987654321
    gen = torch.Generator().manual_seed(g_ch + 10 * per_sample)
    y = torch.randn(n, h, h, c, generator=gen) * 2 + 0.5
    gamma, beta = 0.5 + torch.rand(c, generator=gen), 0.3 * torch.randn(c, generator=gen)
    den = 1.0 + 0.5 * torch.randn(n, c, generator=gen) if with_den else None
    dz = torch.randn(n, h, h, c, generator=gen)
    guide = torch.rand(n, h, h, g_ch, generator=gen) if g_ch else None
    gw = torch.randn(g_ch, c, generator=gen) if g_ch else None
    gb = 0.1 * torch.randn(c, generator=gen) if g_ch else None
    yd = y.cuda()
    d = ops.norm_desc(y.shape, per_sample, c, g_ch, c if g_ch else 0, 0)
    d.dropout_keep, d.dropout_seed = keep, seed
    if leaky:
        d.guide_leaky, d.guide_alpha = 2, 0.0
    flat = yd.reshape(n, h * h, c)
    stats = torch.stack([flat.sum(1), (flat * flat).sum(1)]).contiguous()
    aff = ops.norm_finalize(d, stats, n, gamma.cuda(), beta.cuda(), 1e-6 if per_sample else 1e-3, 0.99, True,
                            torch.zeros(c).cuda(), torch.ones(c).cuda(), yd.device)
    cu = lambda t: None if t is None else t.cuda().contiguous()
    den_k = den if (with_den or not g_ch or leaky) else torch.ones(n, c)      # guide bias sum needs the density variant
    z = torch.empty_like(yd)
    ops.norm_apply_relu(d, yd, aff, z, cu(guide), cu(gw), cu(gb), cu(den_k))
    out = ops.norm_relu_bwd(d, yd, cu(dz), aff, True, True, cu(guide), cu(gw), cu(gb), cu(den_k))
    dy, dgamma, dbeta, dgw, dgb = out[:5]
    mask = torch.from_numpy(unit_mask_host(seed, (n, h, h, c), keep)).double()
    assert 0.6 < (mask > 0).double().mean().item() < 0.8
    d64 = lambda t: None if t is None else t.double().requires_grad_(True)
    y64, g64, b64, den64, gw64, gb64 = d64(y), d64(gamma), d64(beta), d64(den), d64(gw), d64(gb)
    t = tf_ops.instance_norm(y64, g64, b64, eps=1e-6) if per_sample else \
        tf_ops.batch_norm(y64, g64, b64, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64), True)[0]
    u = t * mask
    if den64 is not None:
        u = u * den64[:, None, None, :]
    if g_ch:
        s = guide.double() @ gw64 + gb64
        u = u + (torch.relu(s) if leaky else s)
    ref = torch.relu(u)
    ref.backward(dz.double())
    tol = 2e-5
    assert rel(z.cpu().numpy(), ref.detach().numpy()) < tol
    assert rel(dy.cpu().numpy(), y64.grad.numpy()) < tol
    assert rel(dgamma.cpu().numpy(), g64.grad.numpy()) < tol and rel(dbeta.cpu().numpy(), b64.grad.numpy()) < tol
    if with_den:
        assert rel(out[5].cpu().numpy(), den64.grad.numpy()) < tol
    if g_ch:
        assert rel(dgw.cpu().numpy(), gw64.grad.numpy()) < tol and rel(dgb.cpu().numpy(), gb64.grad.numpy()) < tol


@pytest.mark.parametrize("g_ch", [1, 2])
def test_norm_per_sample_guide_weights_with_relu_branch(g_ch):
    """--fix under instance norm: per-sample folded guide weights gw [N, g, C] / gb [N, C], ReLU on the guide branch;
    dgw / dgb come back per sample."""
    from boxsegliver_amd import ops
    from oracle import tf_ops
    n, h, c = 3, 10, 128
    gen = torch.Generator().manual_seed(g_ch)
    y = torch.randn(n, h, h, c, generator=gen) * 2 + 0.5
    beta = 0.3 * torch.randn(c, generator=gen)
    dz = torch.randn(n, h, h, c, generator=gen)
    guide = torch.rand(n, h, h, g_ch, generator=gen)
    gw = torch.randn(n, g_ch, c, generator=gen)
    gb = 0.3 * torch.randn(n, c, generator=gen)
    yd = y.cuda()
    d = ops.norm_desc(y.shape, True, c, g_ch, c, 0)
    d.guide_leaky, d.guide_alpha, d.guide_per_sample = 2, 0.0, 1
    flat = yd.reshape(n, h * h, c)
    stats = torch.stack([flat.sum(1), (flat * flat).sum(1)]).contiguous()
    aff = ops.norm_finalize(d, stats, n, None, beta.cuda(), 1e-6, 0.0, True, None, None, yd.device)
    z = torch.empty_like(yd)
    ops.norm_apply_relu(d, yd, aff, z, guide.cuda(), gw.cuda(), gb.cuda())
    dy, dgamma, dbeta, dgw, dgb = ops.norm_relu_bwd(d, yd, dz.cuda(), aff, False, True, guide.cuda(), gw.cuda(), gb.cuda())
    assert dgw.shape == (n, g_ch, c) and dgb.shape == (n, c)
    y64, b64, gw64, gb64 = y.double().requires_grad_(True), beta.double().requires_grad_(True), \
        gw.double().requires_grad_(True), gb.double().requires_grad_(True)
    t = tf_ops.instance_norm(y64, None, b64, eps=1e-6)
    s = torch.einsum("nhwg,ngc->nhwc", guide.double(), gw64) + gb64[:, None, None, :]
    ref = torch.relu(t + torch.relu(s))
    ref.backward(dz.double())
    tol = 2e-5
    assert rel(z.cpu().numpy(), ref.detach().numpy()) < tol and rel(dy.cpu().numpy(), y64.grad.numpy()) < tol
    assert rel(dbeta.cpu().numpy(), b64.grad.numpy()) < tol
    assert rel(dgw.cpu().numpy(), gw64.grad.numpy()) < tol and rel(dgb.cpu().numpy(), gb64.grad.numpy()) < tol


def test_guide_moments_exact():
    from boxsegliver_amd import ops
    gen = torch.Generator().manual_seed(2)
    g = torch.rand(3, 16, 20, 2, generator=gen)
    for per_sample in (False, True):
        m = ops.guide_moments(g.cuda(), per_sample).cpu().double()
        gd = g.double().reshape(3, -1, 2) if per_sample else g.double().reshape(1, -1, 2)
        np.testing.assert_allclose(m[:, :2].numpy(), gd.mean(1).numpy(), rtol=1e-6)
        np.testing.assert_allclose(m[:, 2:].reshape(-1, 2, 2).numpy(), torch.einsum("kpi,kpj->kij", gd, gd).numpy() / gd.shape[1],
                                   rtol=1e-6)


def _whole_net_check(model, inputs, net, params, tensors, args, yml, oracle_kw, loss_tol=1e-4, grad_tol=2e-2):
    images, guide, labels = tensors[:3]
    p64 = {k: v.double() for k, v in params.items()}
    kw = dict(kwargs_of(args))
    kw.update({k: (v.double() if torch.is_tensor(v) else v) for k, v in oracle_kw.items()})
    total, _, logits, grads, new_stats = net.loss_and_grads(p64, images.double(), guide.double(), labels, **kw)
    model.params.zero_grad()
    loss = model(inputs, "train", **yml)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - total.item()) < loss_tol * max(1.0, abs(total.item()))
    got = model.layers["logits"].cpu().numpy()
    assert np.abs(got - logits.numpy()).max() < 1e-3
    num = den = 0.0
    for name in model.params.trainable_names():
        g = model.params[name].grad.cpu().numpy().astype(np.float64)
        if model.params.where[name][0] == "reg":
            g = g + args.weight_decay_rate * model.params[name].detach().cpu().numpy().astype(np.float64)
        ref = grads[name].numpy()
        assert np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30) < 0.15, name
        num += np.sum((g - ref) ** 2)
        den += np.sum(ref ** 2)
    assert (num / den) ** 0.5 < grad_tol
    for name, ref in new_stats.items():
        np.testing.assert_allclose(model.params[name].cpu().numpy(), ref.numpy(), rtol=2e-4, atol=1e-6)
    return loss


def _setup_variant(args, yml, oracle_ctor_kw, ctx_len=0, size=32):
    from boxsegliver_amd.NetworksV2.GUNet import GUNet
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    images, labels, _ = make_batch(2, size, size, 3, 3, 1234)
    guide = make_guide(labels, args.guide_channel, 1234)
    gen = torch.Generator().manual_seed(5)
    model = GUNet(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda()}
    context = None
    if ctx_len:
        context = torch.rand(2, ctx_len, generator=gen)
        inputs["context"] = context.cuda()
    model(inputs, "eval", **yml)
    net = gunet2d.GUNet2DOracle(3, 3, guide_channel=args.guide_channel, normalizer=args.normalizer,
                                context_length=ctx_len or None, context_fc_channels=yml["context_fc_channels"], **oracle_ctor_kw)
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.specs]
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias", "fc_b"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        elif "spatial" in name and kind == "conv_w":
            params[name] = 0.5 * torch.randn(t.shape, generator=gen)
        elif kind in ("moving_mean",):
            params[name] = 0.1 * torch.randn(t.shape, generator=gen)
        elif kind in ("moving_var",):
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        else:
            params[name] = t.clone()
    model.params.load_state(params)
    return model, inputs, net, params, (torch.from_numpy(images), torch.from_numpy(guide), torch.from_numpy(labels).long(),
                                        context)


@pytest.mark.parametrize("normalizer,g_ch", [("instance_norm", 1), ("batch_norm", 2)])
def test_gunet_fix_matches_oracle(normalizer, g_ch):
    """--fix: the oracle materialises conv1x1 -> norm -> ReLU on the guide; the product folds the norm into the guide weights
    from the guide's moments.  Same loss / logits / gradients (incl. the guide convs' gamma / beta) and moving statistics."""
    args = make_args(normalizer=normalizer, guide_channel=g_ch, fix=True)
    model, inputs, net, params, tensors = _setup_variant(args, YML, dict(fix=True))
    names = list(model.params.state_dict())
    ns = "BatchNorm" if normalizer == "batch_norm" else "InstanceNorm"
    assert "GUNet/spatial/conv2/{}/gamma".format(ns) in names and "GUNet/spatial/conv2/biases" not in names
    _whole_net_check(model, inputs, net, params, tensors, args, YML, {})
    # eval mode: batch norm uses the moving statistics of the guide convs
    logits_eval, _ = net.forward({k: v.double() for k, v in model.params.state_dict().items()}, tensors[0].double(),
                                 tensors[1].double(), False)
    model(inputs, "eval", **YML)
    assert np.abs(model.layers["logits"].cpu().numpy() - logits_eval.numpy()).max() < 1e-3


@pytest.mark.parametrize("normalizer,use_context", [("instance_norm", False), ("batch_norm", True)])
def test_gunet_dropout_matches_oracle(normalizer, use_context):
    """--dropout 0.3: the first conv unit of every encoder block is masked after its norm; the oracle gets the masks the
    kernels regenerate (restated RNG), so the comparison is on the arithmetic."""
    yml = dict(YML, context_fc_channels=[32, 16])
    args = make_args(normalizer=normalizer, dropout=0.3, use_context=use_context, side_dropout=0.0)
    model, inputs, net, params, tensors = _setup_variant(args, yml, {}, ctx_len=10 if use_context else 0)
    calls = getattr(model, "_dropout_calls", 0)
    masks = {}
    for i in range(5):                                   # the seeds GUNet._build_network will use in the next training call
        c = 64 * 2 ** i
        # (the context MLP draws one call number per forward before the encoder does)
        seed = int(args.seed) * 7919 + (calls + 1 + i + (1 if use_context else 0)) * 131 + i
        masks["GUNet/Encode/down_conv{}/mod_conv1".format(i + 1)] = torch.from_numpy(
            unit_mask_host(seed, (2, 32 >> i, 32 >> i, c), 0.7))
    okw = {"unit_masks": masks}
    if use_context:
        okw["context"] = tensors[3]
    _whole_net_check(model, inputs, net, params, tensors, args, yml, okw)
    model(inputs, "eval", **yml)                          # no dropout outside training
    okw_eval = {k: v for k, v in okw.items() if k != "unit_masks"}
    p64 = {k: v.double() for k, v in model.params.state_dict().items()}
    ref, _ = net.forward(p64, tensors[0].double(), tensors[1].double(), False,
                         context=okw_eval.get("context").double() if use_context else None)
    assert np.abs(model.layers["logits"].cpu().numpy() - ref.numpy()).max() < 1e-3


@pytest.mark.parametrize("normalizer", ["instance_norm", "batch_norm"])
def test_gunet_use_se_matches_oracle(normalizer):
    """--use_se: gains = sigmoid(fc(relu(fc(concat(mean_hw(norm(conv)), context slice))))) per modulated conv unit; under batch
    norm the pooled value depends on the unit's own conv output (the extra term of unetk_norm_se_bwd_add)."""
    yml = dict(YML, context_fc_channels=[32, 16])
    args = make_args(normalizer=normalizer, use_context=True, use_se=True, side_dropout=0.0)
    model, inputs, net, params, tensors = _setup_variant(args, yml, dict(use_se=True), ctx_len=10)
    names = list(model.params.state_dict())
    assert "GUNet/Encode/down_conv2/mod_conv1/fully_connected/weights" in names
    assert model.params["GUNet/Encode/down_conv2/mod_conv1/fully_connected/weights"].shape == (128 + 16, (128 + 16) // 4)
    assert model.params["GUNet/context/fc3/weights"].shape == (16, 16 * 4 * 2)
    _whole_net_check(model, inputs, net, params, tensors, args, yml, {"context": tensors[3]})


# ----------------------------------------------------------------------------- 1-D VGG context models (GUNet_DE_VGG16{B,D}.yml)
@pytest.mark.parametrize("k,length,cin,cout,relu", [(3, 37, 1, 2, True), (3, 16, 8, 16, True), (1, 9, 16, 16, True),
                                                    (3, 5, 4, 6, False)])
def test_conv1d_and_same_maxpool1d_against_float64_autograd(k, length, cin, cout, relu):
    """slim.conv1d (SAME, bias, ReLU) and tf.layers.max_pooling1d(2, 2, "same") of slim_nets.vgg16* (slim_nets.py:60-144)."""
    from boxsegliver_amd import ops
    gen = torch.Generator().manual_seed(11)
    b = 3
    x = torch.randn(b, length, cin, generator=gen)
    w = torch.randn(k, cin, cout, generator=gen) / (k * cin) ** 0.5
    bias = 0.3 * torch.randn(cout, generator=gen)
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, bias))
    y = ops.Conv1d.apply(xd, wd, bd, relu)
    z = ops.MaxPool1d.apply(y)
    assert z.shape == (b, (length + 1) // 2, cout)
    dz = torch.randn(z.shape, generator=gen)
    z.backward(dz.cuda())
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    t = torch.nn.functional.conv1d(x64.permute(0, 2, 1), w64.permute(2, 1, 0), b64, padding=(k - 1) // 2)
    t = torch.relu(t) if relu else t
    ref = torch.nn.functional.max_pool1d(t, 2, 2, ceil_mode=True).permute(0, 2, 1)
    ref.backward(dz.double())
    assert rel(z.detach().cpu().numpy(), ref.detach().numpy()) < 1e-6
    for got, want in ((xd.grad, x64.grad), (wd.grad, w64.grad), (bd.grad, b64.grad)):
        assert rel(got.cpu().numpy(), want.numpy()) < 1e-5


@pytest.mark.parametrize("cmodel,normalizer", [("vgg16B", "instance_norm"), ("vgg16D", "batch_norm"), ("vgg16C", "instance_norm")])
def test_gunet_vgg_context_models_match_oracle(cmodel, normalizer):
    """context_model vgg16B / vgg16D (the shipped ext_config/GUNet_DE_VGG16{B,D}.yml) and vgg16C (GUNet.py:62-75): variable
    names and shapes, the zeros / ones initialisation of the last layer (every gain = 1), and -- with random variables --
    loss, logits, the gains and all context-branch gradients against the float64 oracle."""
    import yaml
    from pathlib import Path
    from boxsegliver_amd import ops
    from boxsegliver_amd.NetworksV2.GUNet import GUNet
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    cfg_name = "GUNet_DE_VGG16B.yml" if cmodel != "vgg16D" else "GUNet_DE_VGG16D.yml"
    cfg = yaml.safe_load((Path(ops.__file__).parent / "NetworksV2" / "ext_config" / cfg_name).read_text())
    assert cfg["context_conv_init_channels"] == 2 and cfg["context_fc_channels"] == [200, 200]
    cfg["context_model"] = cmodel
    yml = dict(cfg, build_metrics=True, build_summaries=False)
    ctx_len = 45                                                           # odd lengths exercise the "same" pools
    args = make_args(normalizer=normalizer, use_context=True, use_spatial=True, side_dropout=0.0)
    images, labels, _ = make_batch(2, 32, 32, 3, 3, 1234)
    guide = make_guide(labels, args.guide_channel, 1234)
    gen = torch.Generator().manual_seed(21)
    context = torch.rand(2, ctx_len, generator=gen)
    model = GUNet(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda(), "context": context.cuda()}
    model(inputs, "eval", **yml)
    net = gunet2d.GUNet2DOracle(3, 3, guide_channel=1, normalizer=normalizer, context_length=ctx_len,
                                context_fc_channels=(200, 200), context_model=cmodel, context_conv_init_channels=2)
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.specs]
    names = list(model.params.state_dict())
    assert "GUNet/context/conv1/conv1_1/weights" in names and "GUNet/context/fc8/biases" in names and "GUNet/context/fc1/weights" not in names
    assert ("GUNet/context/conv3_3/weights" in names) == (cmodel == "vgg16C")
    assert ("GUNet/context/conv5/conv5_3/weights" in names) == (cmodel == "vgg16D")
    assert model.params["GUNet/context/conv1/conv1_1/weights"].shape == (3, 1, 2)
    assert model.params["GUNet/context/fc6/weights"].shape == (2 * 16, 200)             # ceil(45 / 32) = 2 positions x 16 channels
    assert float(model.params["GUNet/context/fc8/weights"].abs().sum()) == 0.0 and \
        float((model.params["GUNet/context/fc8/biases"] - 1).abs().sum()) == 0.0          # GUNet.py:73-74
    assert torch.equal(model.layers["context_params"], torch.ones_like(model.layers["context_params"]))
    assert model.params.where["GUNet/context/conv2/conv2_1/weights"][0] == "noreg"       # slim.conv1d: no regulariser in scope
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias", "fc_b"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        elif "spatial" in name:
            params[name] = 0.5 * torch.randn(t.shape, generator=gen)
        elif kind == "fc_w_zero":
            params[name] = torch.randn(t.shape, generator=gen) * (2.0 / t.shape[0]) ** 0.5
        elif kind == "conv1d_w":
            params[name] = torch.randn(t.shape, generator=gen) * (2.0 / (t.shape[0] * t.shape[1])) ** 0.5
        else:
            params[name] = t.clone()
    model.params.load_state(params)
    model.params.zero_grad()
    loss = model(inputs, "train", **yml)
    loss.backward()
    torch.cuda.synchronize()
    kw = dict(kwargs_of(args), context=context.double(), drop_masks=None)
    p64 = {k: v.double() for k, v in params.items()}
    total, _, logits, grads64, _ = net.loss_and_grads(p64, torch.from_numpy(images).double(), torch.from_numpy(guide).double(),
                                                      torch.from_numpy(labels).long(), **kw)
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    assert np.abs(model.layers["logits"].cpu().numpy() - logits.numpy()).max() < 1e-3
    den_ref = net.context_params(p64, context.double()).numpy()
    assert rel(model.layers["context_params"].detach().cpu().numpy(), den_ref) < 1e-5
    for name in model.params.trainable_names():
        if "/context/" not in name:
            continue
        g = model.params[name].grad.cpu().numpy()
        ref = grads64[name].numpy()
        assert np.abs(ref).max() > 0, name
        # the density gradient the trunk receives carries the encoder's ReLU flips: compare like the other context tests
        assert rel(g, ref) < 3e-2, (name, rel(g, ref))


# ----------------------------------------------------------------------------- ct_conv (`_context_subnets_conv`, GUNet.py:83-116)
@pytest.mark.parametrize("normalizer", ["instance_norm", "batch_norm"])
def test_gunet_conv_context_subnet_matches_oracle(normalizer):
    """args.ct_conv present (the nf2 pipeline, input_pipeline_iin.py:95): the context is a [bs, 32, 32, 3] image that goes
    through three conv units of the model's arg_scope, a spatial mean and two he_normal fully-connected layers."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.NetworksV2.GUNet import GUNet
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    args = make_args(normalizer=normalizer, use_context=True, use_spatial=True, side_dropout=0.0)
    args.ct_conv = 1
    images, labels, _ = make_batch(2, 32, 32, 3, 3, 1234)
    guide = make_guide(labels, args.guide_channel, 1234)
    gen = torch.Generator().manual_seed(33)
    context = torch.rand(2, 32, 32, 3, generator=gen)
    # spatial mean at op level first
    xm = torch.randn(3, 5, 7, 130, generator=gen)
    xd = xm.cuda().requires_grad_(True)
    ym = ops.SpatialMean.apply(xd)
    gm = torch.randn(3, 130, generator=gen)
    ym.backward(gm.cuda())
    assert rel(ym.detach().cpu().numpy(), xm.double().mean(dim=(1, 2)).numpy()) < 1e-6
    assert rel(xd.grad.cpu().numpy(), (gm.double()[:, None, None, :] / 35).expand(3, 5, 7, 130).numpy()) < 1e-6
    model = GUNet(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda(), "context": context.cuda()}
    model(inputs, "eval", **YML)
    net = gunet2d.GUNet2DOracle(3, 3, guide_channel=1, normalizer=normalizer, context_length=3, context_model="ct_conv")
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.specs]
    names = list(model.params.state_dict())
    assert "GUNet/context/Conv_2/weights" in names and "GUNet/context/fully_connected_1/biases" in names
    assert model.params["GUNet/context/fully_connected_1/weights"].shape == (200, 64 * (2 + 4 + 8 + 16) * 2)
    assert model.params.where["GUNet/context/Conv_1/weights"][0] == "reg"            # slim.conv2d of the model's arg_scope
    params = {}
    for name, t in model.params.state_dict().items():
        kind = net.kinds[name]
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(t.shape, generator=gen)
        elif kind in ("beta", "bias", "fc_b"):
            params[name] = 0.2 * torch.randn(t.shape, generator=gen)
        elif "spatial" in name:
            params[name] = 0.5 * torch.randn(t.shape, generator=gen)
        else:
            params[name] = t.clone()
    params["GUNet/context/fully_connected_1/biases"] = params["GUNet/context/fully_connected_1/biases"] + 1.0
    model.params.load_state(params)
    model.params.zero_grad()
    loss = model(inputs, "train", **YML)
    loss.backward()
    torch.cuda.synchronize()
    kw = dict(kwargs_of(args), context=context.double(), drop_masks=None)
    p64 = {k: v.double() for k, v in params.items()}
    total, _, logits, grads64, new_stats = net.loss_and_grads(p64, torch.from_numpy(images).double(),
                                                              torch.from_numpy(guide).double(),
                                                              torch.from_numpy(labels).long(), **kw)
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    assert np.abs(model.layers["logits"].cpu().numpy() - logits.numpy()).max() < 1e-3
    assert rel(model.layers["context_params"].detach().cpu().numpy(), net.last_context_params.detach().numpy()) < 1e-5
    for name in model.params.trainable_names():
        if "/context/" not in name:
            continue
        g = model.params[name].grad.cpu().numpy().astype(np.float64)
        ref = grads64[name].numpy()
        # (backward() leaves the DATA-loss gradient; the regulariser's wd * w is added inside the optimiser kernel and is
        #  1e-5 * w here, far under the bar)
        assert np.abs(ref).max() > 0, name
        l2 = np.linalg.norm(g - ref) / np.linalg.norm(ref)
        assert l2 < 5e-2, (name, l2)
    for name, ref in new_stats.items():
        if "/context/" in name:
            np.testing.assert_allclose(model.params[name].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)
