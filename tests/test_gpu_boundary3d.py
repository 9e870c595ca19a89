"""GPU: `unetk_boundary_weights3d` (csrc/weights.hip; include/unetk.h) through the C ABI in guarded buffers
against the numpy / scipy restatement (boundary3d_ref.py), then `--loss_weight_type boundary` through UNet3D.

The squared distances are integers and compare exactly.  The map compares with the float64 restatement at rtol 2e-6: that is
small_ops_cases.BOUNDARY_RTOL, set for the 2-D kernel (test_gpu_ops.py::test_boundary_weights_match_oracle_incl_single_label_slice),
and the per-voxel arithmetic here is the same -- one float32 sqrt of an exact integer, a division, expf, an addition, and one
multiplication by the float32 scale of a sum that is taken in double.  Measured on an MI355X, 2026-10-21: at most 1.4e-7 on the
map and 6.2e-8 on a sample's mean (the tests print every row's figure before they assert)."""
import argparse
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import boundary3d_ref as bref
import guardbuf

pytestmark = pytest.mark.gpu

BOUNDARY_RTOL = 2e-6
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
KERNELS = ["b3_x_kernel", "b3_axis_kernel<false>", "b3_axis_kernel<true>", "b3_normalise_kernel"]
# the issue's volumes, then one per block / tile size of the kernels with the extent just past it (the sizes
# of the two shared passes are the constants of csrc/edt_int.h):
#   (3, 9, 65)   W = 65: a second ballot word of b3_x_kernel and a second 64-column strip of b3_axis_kernel; 27 lines per sample,
#                no multiple of the 4 lines of a block of b3_x_kernel (B3_LINES of csrc/weights.hip)
#   (5, 17, 6)   H = 17 and (17, 5, 6) D = 17: a second block of 16 outputs along the axis of b3_axis_kernel (IEDT_T)
#   (3, 129, 4)  H = 129 and (129, 3, 4) D = 129: a second staging chunk of 128 rows (IEDT_STAGE)
VOLUMES = [(6, 20, 24), (10, 32, 40), (4, 70, 9), (1, 33, 65), (3, 5, 300), (2, 300, 5), (70, 6, 7), (5, 1, 70), (1, 1, 1), (2, 1, 1),
           (3, 9, 65), (5, 17, 6), (17, 5, 6), (3, 129, 4), (129, 3, 4)]
SCALES = (1, 3)


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    lib()
    return _ops


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(b):
    return None if b is None else ctypes.c_void_p(b.ptr())


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return out, [n.replace(" ", "").replace("(anonymousnamespace)::", "") for n in ops.profile_read()[1]]


def ws_bytes(n, d, h, w):
    """include/unetk.h: one double per block of the z pass (64 columns x 16 slices of a row), then the int32 field between the y
    and the z pass."""
    return 8 * n * h * ((w + 63) // 64) * ((d + 15) // 16) + 4 * n * d * h * w


def _i32(g):
    return g.view.clone().view(torch.int32).cpu().numpy()


def run(ops, lab, k, want_d2=True):
    """The entry in guarded buffers, traced, twice: -> (wmap float32, d2 int32 or None), numpy [N, D, H, W]."""
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    n, d, h, w = lab.shape
    labels = guardbuf.guarded_input(torch.from_numpy(lab).cuda().view(torch.float32))    # int32 bits in an fp32 guarded buffer
    wmap = guardbuf.guarded((n, d, h, w))
    d2 = guardbuf.guarded((n, d, h, w)) if want_d2 else None
    nbytes = int(lib().unetk_boundary_weights3d_ws_bytes(n, d, h, w))
    assert nbytes == ws_bytes(n, d, h, w)
    ws = guardbuf.GuardedWorkspace(nbytes)
    call = lambda: lib().unetk_boundary_weights3d(_p(labels), n, d, h, w, k, _p(wmap), _p(d2), _p(ws), nbytes, _stream())
    outs = [o for o in (wmap, d2) if o is not None]

    def check(what):
        for o in outs:
            assert o.check_untouched(), what + ": wrote outside an output"
            assert o.unwritten() == 0, what + ": left output elements unwritten"
        assert labels.changed_anywhere() == 0, what + ": changed the labels"
        assert ws.guard_intact(), what + ": wrote outside the workspace"

    ws.fill(0xFF)                                                # NaN patterns: nothing may be read before it is written
    rc, names = _trace(ops, call)
    assert rc == 0, rc
    assert len(names) == len(KERNELS) and all(e in g for e, g in zip(KERNELS, names)), names
    check("first run")
    first = [o.bits().clone() for o in outs]
    for o in outs:
        o.reset()
    ws.fill(0xFF)
    assert call() == 0
    torch.cuda.synchronize()
    check("second run")
    for o, f in zip(outs, first):
        assert torch.equal(o.bits(), f), "not bit-reproducible"
    return wmap.view.clone().cpu().numpy(), (_i32(d2) if want_d2 else None)


def _check_map(got, lab, k, what):
    want = bref.weights(lab, k)
    rel = np.abs(got.astype(np.float64) - want) / want
    mean = got.astype(np.float64).mean(axis=(1, 2, 3))
    print(what, "map rel", rel.max(), "mean - 1", np.abs(mean - 1.0).max())
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=BOUNDARY_RTOL, err_msg=what)
    np.testing.assert_allclose(mean, 1.0, rtol=0, atol=1e-6, err_msg=what)


# ------------------------------------------------------------------------------------------------- exact rows
@pytest.mark.parametrize("shape", VOLUMES, ids=["x".join(map(str, s)) for s in VOLUMES])
def test_exact_rows(ops, shape):
    """Two samples per volume (the ellipsoids sit on the first slice of one and on the last of the other); both scales."""
    lab = bref.labels(shape, 100 + sum(shape), n=2)
    want = {k: bref.d2(lab, k) for k in SCALES}
    if shape[0] >= 3:                                            # both passes must matter -- asserted on the reference alone
        for i in range(2):
            other = bref.other_slice(lab[i])
            assert other.mean() >= 0.15, (shape, i, other.mean())
            assert (want[3][i][other] != want[1][i][other]).all(), (shape, i)
    for k in SCALES:
        wmap, d2 = run(ops, lab, k)
        bad = d2 != want[k]
        assert not bad.any(), "{} K={}: {} of {} voxels differ, first at {}".format(shape, k, int(bad.sum()), bad.size,
                                                                                  np.argwhere(bad)[:3].tolist())
        _check_map(wmap, lab, k, "{} K={}".format(shape, k))
    if shape == (1, 1, 1):
        assert (want[1] == -1).all()                             # a single voxel has no ring: the rule for ring-free samples


def test_far_from_a_single_voxel(ops):
    """(2, 8, 600) with one foreground voxel at x = 0: distances run past 417, where the weight is exactly 1 in float32 -- a
    search windowed by distance would show here."""
    lab = np.zeros((1, 2, 8, 600), np.int32)
    lab[0, 0, 3, 0] = 1
    want = bref.d2(lab, 1)
    assert want.max() > 417 ** 2
    wmap, d2 = run(ops, lab, 1)
    np.testing.assert_array_equal(d2, want)
    _check_map(wmap, lab, 1, "single voxel")


def test_without_d2_out_and_through_the_wrapper(ops):
    lab = bref.labels((6, 20, 24), 7, n=2)
    with_d2, d2 = run(ops, lab, 3)
    without, none = run(ops, lab, 3, want_d2=False)
    assert none is None and np.array_equal(with_d2.view(np.int32), without.view(np.int32))
    t = torch.from_numpy(lab).cuda()
    wmap, d2w = ops.boundary_weights3d(t, 3, want_d2=True)
    assert np.array_equal(wmap.cpu().numpy().view(np.int32), with_d2.view(np.int32)) and np.array_equal(d2w.cpu().numpy(), d2)
    assert torch.equal(ops.boundary_weights3d(t, 3), wmap)
    assert torch.equal(ops.boundary_weights3d(t.long(), z_scale=3), wmap)       # int64 labels, as the input pipeline's
    with pytest.raises(ValueError):
        ops.boundary_weights3d(t[0])


# ------------------------------------------------------------------------------------------------- the bits before the shared core
def _load_generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_edt_fixture.py")
    spec = importlib.util.spec_from_file_location("make_edt_fixture", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_map_bits_are_those_before_the_shared_edt_core(ops):
    """tests/golden/edt_maps_before.npz holds the map's float32 bits as weights.hip computed them with its own copy of the two
    integer passes and of the tree sum (recorded by tests/golden/make_edt_fixture.py on an MI355X): moving onto csrc/edt_int.h
    and b3_block_sum changed no bit -- not the minima, not the order of the double sums."""
    G = _load_generator()
    z = np.load(G.OUT)
    assert sorted(z.files) == sorted(G.key(s, k) for s in G.SHAPES for k in G.SCALES), "the fixture was recorded for other cases"
    for shape in G.SHAPES:
        for k in G.SCALES:
            got, want = G.record(ops, shape, k), z[G.key(shape, k)]
            assert want.dtype == np.uint32 and want.shape == (2,) + shape
            bad = got != want
            assert np.array_equal(got, want), "{} K={}: {} of {} words differ, first at {}".format(
                shape, k, int(bad.sum()), bad.size, np.argwhere(bad)[:3].tolist())


# ------------------------------------------------------------------------------------------------- batch isolation
def test_batch_isolation(ops):
    """N = 3: a ring-bearing sample, a single-label sample, and a sample whose labels differ only in its first slice (its ring
    lies in its first two slices, next to the single-label sample before it in memory: a 3x3x3 ring always reaches the
    neighbouring slice)."""
    shape = (6, 20, 24)
    a = bref.labels(shape, 5)[0]
    b = np.full(shape, 1, np.int32)
    c = np.zeros(shape, np.int32)
    c[0, 4:9, 10:17] = 2
    assert bref.ring(c)[:2].any() and not bref.ring(c)[2:].any()
    for k in SCALES:
        wmap, d2 = run(ops, np.stack([a, b, c]), k)
        assert (d2[1] == -1).all() and (wmap[1] == 1.0).all()
        for i, lab in ((0, a), (2, c)):
            w1, q1 = run(ops, lab[None], k)
            assert np.array_equal(q1[0], d2[i]) and np.array_equal(w1[0].view(np.int32), wmap[i].view(np.int32)), (k, i)
        np.testing.assert_array_equal(d2, bref.d2(np.stack([a, b, c]), k))


# ------------------------------------------------------------------------------------------------- D = 1 against the 2-D kernel
def test_depth_one_against_the_2d_kernel(ops):
    """On a ring-bearing slice the 3-D entry computes what unetk_boundary_weights computes.  Not bit for bit: the 2-D kernel adds a
    whole image row in float32 (256 thread sums, then a tree) and the rows in double, the 3-D one adds the four weights of a
    thread and the 256 threads of a 64 x 16 block in double -- other partial sums, so the scale may differ in its last bits.  Both
    lie within 2e-6 of float64, and so of each other within twice that; the unscaled ratio to a reference voxel needs none of
    this, but the scale is part of what a user gets.  (On this slice the two came out bit-equal; nothing promises it.)"""
    lab = bref.labels((1, 33, 65), 21, n=2)
    w3, _ = run(ops, lab, 1)
    w2 = ops.boundary_weights(torch.from_numpy(lab[:, 0]).cuda()).cpu().numpy()
    rel = np.abs(w3[:, 0].astype(np.float64) - w2) / w2
    print("3-D at D = 1 against the 2-D kernel: rel", rel.max())
    np.testing.assert_allclose(w3[:, 0], w2, rtol=BOUNDARY_RTOL)


# ------------------------------------------------------------------------------------------------- refusals
REFUSALS = [("z_scale_0", dict(k=0), E_UNSUPPORTED), ("z_scale_17", dict(k=17), E_UNSUPPORTED), ("d_1025", dict(d=1025), E_UNSUPPORTED),
            ("w_4097", dict(w=4097), E_UNSUPPORTED), ("ws_16_bytes_short", dict(short=16), E_WORKSPACE), ("null_wmap", dict(null="wmap"), E_BADARG),
            ("null_labels", dict(null="labels"), E_BADARG), ("null_ws", dict(null="ws"), E_BADARG), ("n_0", dict(n=0), E_BADARG)]


@pytest.mark.parametrize("name,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(ops, name, over, code):
    """Buffers of the ordinary (valid) size: a refused call, however large its extents, launches nothing and writes nothing."""
    n, d, h, w = 2, 3, 4, 5
    labels = guardbuf.guarded_input(torch.zeros((n, d, h, w), device="cuda"))
    wmap, d2 = guardbuf.guarded((n, d, h, w)), guardbuf.guarded((n, d, h, w))
    nbytes = ws_bytes(n, d, h, w)
    ws = guardbuf.GuardedWorkspace(nbytes)
    bufs = dict(labels=labels, wmap=wmap, ws=ws)
    ptrs = {key: (None if over.get("null") == key else _p(b)) for key, b in bufs.items()}
    rc, names = _trace(ops, lambda: lib().unetk_boundary_weights3d(
        ptrs["labels"], over.get("n", n), over.get("d", d), h, over.get("w", w), over.get("k", 1), ptrs["wmap"], _p(d2), ptrs["ws"],
        nbytes - over.get("short", 0), _stream()))
    assert rc == code and names == [], (name, rc, names)
    assert wmap.changed_anywhere() == 0 and d2.changed_anywhere() == 0 and labels.changed_anywhere() == 0, name
    assert ws.guard_intact() and torch.equal(ws.buf, ws.snap), name
    for dd, ww in ((1025, w), (d, 4097)):
        assert lib().unetk_boundary_weights3d_ws_bytes(n, dd, h, ww) == 0


# ------------------------------------------------------------------------------------------------- through the net
# the smallest UNet3D shape of tests/test_gpu_unet3d.py, its make_args / setup restated
YML = dict(init_channels=30, max_channels=320, num_pool_layers=4, ret_prob=False, ret_pred=True, build_metrics=True,
           build_summaries=False)


def make_args(**over):
    a = argparse.Namespace(
        classes=["NF"], batch_size=2, num_gpus=1, im_depth=4, im_height=32, im_width=32, im_channel=1,
        normalizer="instance_norm", without_norm=False, weight_init="xavier", weight_decay_rate=3e-5, bias_decay=False,
        loss_type="xentropy", loss_weight_type="boundary", loss_numeric_w=[1.0, 1.0], loss_proportion_decay=1000,
        metrics_train=["Dice"], img_grad=False, tag="test3d", seed=1234, use_spatial=False, guide_channel=2,
        learning_rate=3e-4, learning_policy="period_step", lr_decay_step=100000, lr_decay_rate=0.1,
        num_of_total_steps=1000, lr_power=0.9, lr_end=1e-6, lr_decay_boundaries=None, lr_custom_values=None,
        optimizer="Adam", eval_per_epoch=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _batch():
    from boxsegliver_amd.data.synthetic import make_batch_3d
    images, labels, _ = make_batch_3d(2, 4, 32, 32, 1, 2, 1234)
    return images, labels


def _params(net):
    from oracle import unet3d
    params = unet3d.init_params(net.specs, seed=5)
    g = torch.Generator().manual_seed(9)
    for name, _, kind in net.specs:
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(params[name].shape, generator=g)
        elif kind in ("beta", "bias"):
            params[name] = 0.1 * torch.randn(params[name].shape, generator=g)
    return params


def _model(args, params):
    from boxsegliver_amd.NetworksV2.UNet3D import UNet3D
    images, labels = _batch()
    model = UNet3D(args)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda()}
    model(inputs, "eval", **YML)
    model.params.load_state(params)
    return model, inputs


def _step(model, inputs):
    model.params.zero_grad()
    loss = model(inputs, "train", **YML)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), model.params.grad["reg"].clone(), model.params.grad["noreg"].clone()


@pytest.fixture(scope="module")
def oracle():
    """float64, once: the logits of UNet3DOracle.forward, the cross-entropy per voxel weighted by the restatement's map
    (sum(w ce) / count(w != 0), K = 1 and K = 2), the regulariser, and autograd's gradients of the K = 1 loss."""
    import torch.nn.functional as F

    from oracle import unet3d
    images, labels = _batch()
    assert bref.ring(labels[0]).any() and bref.ring(labels[1]).any()
    net = unet3d.UNet3DOracle(1, 2, normalizer="instance_norm")
    params = _params(net)
    p64 = {}
    for name, t in params.items():
        p64[name] = t.double().requires_grad_(net.kinds[name] in unet3d.TRAINABLE_KINDS)
    logits, _ = net.forward(p64, torch.from_numpy(images).double(), True)
    lab = torch.from_numpy(labels).long()
    ce = F.cross_entropy(logits.reshape(-1, 2), lab.reshape(-1), reduction="none").reshape(lab.shape)
    reg = net.regularization_loss(p64, 3e-5)
    total = {}
    for k in (1, 2):
        w = torch.from_numpy(bref.weights(labels, k))
        total[k] = (w * ce).sum() / float((w != 0).sum()) + reg
    total[1].backward()
    grads = {n: t.grad.detach() for n, t in p64.items() if t.requires_grad}
    return dict(net=net, params=params, total={k: v.item() for k, v in total.items()}, grads=grads)


def test_boundary_loss_through_unet3d(ops, oracle):
    args = make_args()
    model, inputs = _model(args, oracle["params"])
    assert [(n, tuple(s), k) for n, s, k in oracle["net"].specs] == [(n, tuple(s), k) for n, s, k in model.params.logical_specs]
    (loss, greg, gnoreg), names = _trace(ops, lambda: _step(model, inputs))
    assert [sum(k in n for n in names) for k in KERNELS] == [1, 1, 1, 1], names  # the map is built once per step
    want = oracle["total"][1]
    print("loss", loss, "float64", want)
    assert abs(loss - want) < 1e-4 * max(1.0, abs(want))
    num = den = 0.0
    for name in model.params.trainable_names():
        g = model.params.logical_grad(name).numpy().astype(np.float64)
        ref = oracle["grads"][name].numpy()
        num += np.sum((g - ref) ** 2)
        den += np.sum(ref ** 2)
    print("gradient rel L2", (num / den) ** 0.5)
    assert (num / den) ** 0.5 < 1e-2
    # the same step on a caller's map: identical bits
    given = dict(inputs, pixel_weights=ops.boundary_weights3d(inputs["labels"]))
    loss_g, greg_g, gnoreg_g = _step(model, given)
    assert loss_g == loss and torch.equal(greg_g, greg) and torch.equal(gnoreg_g, gnoreg)
    # --boundary_z_scale 2: another map, another loss -- the float64 one of K = 2
    args.boundary_z_scale = 2
    loss2 = _step(model, inputs)[0]
    want2 = oracle["total"][2]
    assert want2 != want and loss2 != loss and abs(loss2 - want2) < 1e-4 * max(1.0, abs(want2))


def test_other_weight_types_launch_nothing_new(ops, oracle):
    model, inputs = _model(make_args(loss_weight_type="numerical"), oracle["params"])
    _, names = _trace(ops, lambda: _step(model, inputs))
    assert names and not any("b3_" in n for n in names), [n for n in names if "b3_" in n]
    with pytest.raises(ValueError, match="2-D labels only"):                     # a caller that comes without a map
        from boxsegliver_amd import loss_metrics
        loss_metrics.build_head_desc(make_args(), 2, 4096, 32, 2)


def test_boundary_loss_under_bf16c(oracle):
    """--compute_dtype bf16c runs and agrees with fp32 to rtol 3e-2, the tolerance between the two modes' losses in
    tests/test_gpu_unet3d_bf16c.py::test_unet3d_bf16c_trains_beside_fp32_and_keeps_the_padding_zero."""
    losses = {}
    for mode in ("fp32", "bf16c"):
        model, inputs = _model(make_args(compute_dtype=mode), oracle["params"])
        losses[mode] = _step(model, inputs)[0]
    print(losses)
    assert np.isfinite(losses["bf16c"])
    np.testing.assert_allclose(losses["bf16c"], losses["fp32"], rtol=3e-2)
