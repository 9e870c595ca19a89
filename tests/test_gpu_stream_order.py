"""GPU: every hand-off between streams, and between the host and the device, with one side of it held back (stream_delay.py).

The hand-offs:
  * filter gradients on the side stream (ops._on_side): side.wait_stream(main) before the side kernel reads dy;
    record_stream on dy / x / the transposed conv's scratch; the engine callback side_join at the end of backward; the
    side_join() of GradBuckets._launch; the side_join() of ops.new_step after a backward that raised; no main-stream kernel
    writing dy or x in place after the side launch (norm_se_bwd_add* write dy in place BEFORE it);
  * utils/volume_writer.VolumeWriter.submit: the copy stream, its `ready` and `done` events, flat.record_stream, two pinned
    buffers reused by slot;
  * data/lits.SliceStore: two pinned staging buffers refilled by host threads behind done[slot].synchronize();
  * the propagation evaluator's pinned obj_host / table_host behind the one synchronize() per slice;
  * per-step tables uploaded from fresh pinned memory with non_blocking=True.

Each test runs the same computation on one stream (or undelayed) and with one stream held for D = max(4 * T, 20 ms), T measured
in the same test on the undelayed run, and compares bit for bit (torch.equal, file bytes): no tolerances.  A missing wait
reads a stale value on every run.  test_control_* shows on project code that the comparison can fail.

The held stream must be one that runs BESIDE the main stream.  HIP maps streams onto a few hardware queues and torch hands
them out from a pool, so late in a long pytest process a fresh torch.cuda.Stream() can share the main stream's queue: holding
it then holds the main stream too (seen in the whole-suite run, where the self-check read the NEW value without waiting, while
the module alone passed).  The tests therefore give ops._Side and the volume writer a stream that stream_delay has probed
(independent_streams); which stream the product picks is not changed.

Seen on the MI355X (pytest -s prints one "stream-order ..." line per case; T and D in ms, launches summed over the case's
backwards -- three under late-side, two under late-main):
  harness          torch.cuda._sleep counts 2.40e6 cycles per ms (the shader clock); 40 ms asked, 40.00 ms measured
  unet-fp32        T 6.9  D 27.7  conv2d 51 deconv 12      unet-bf16   T 4.9  D 20    same      unet-bf16c  T 4.1  D 20   same
  unet-fp32-wgrad-after-dgrad   T 9.3  D 37.3  51 / 12     unet-fp32-deconv-on-main     T 5.5  D 22.1  51 / 0
  gunet-batch-norm T 5.9  D 23.5  51 / 12    gunet-instance-norm  T 6.3  D 25.1  51 / 12    gunet-se-dropout  T 15.4  D 61.5  51 / 12
  lgnet            T 6.3  D 25.4  51 / 12    interunet  T 8.5  D 34.0  54 / 0               smallunet  T 7.5  D 30.0  45 / 9
  unet3d-fp32      T 6.6  D 26.3  conv3d 51 deconv 12 (7.0 / 27.3 with the filter gradient behind the input gradient)
  unet3d-bf16c     T 5.8  D 23.1  conv3d 51 deconv 12 (5.8 / 23.0)
  raised backward  T 7.3  D 29.2  14 conv2d and 4 deconv launches before the hook raised
  bucket           T 3.7  D 20    5 buckets, 4 launched from inside backward, 5 holds (one after every join)
  volume writer    T 1.0 / 0.6  D 20      slice store  T 3.6  D 20      pinned tables  T 0.6  D 20
  propagation      D 3 per call, 32 slices, at most 2 objects (72 in the grown case)
One local run each of four one-line mutations (none committed; each only makes values stale): without
side.wait_stream(main) every test_late_main_* case fails; without the wait in side_join every test_late_side_* case, the
raised-backward and the bucket test fail; without dy's / the scratch's record_stream every test_late_side_* case (and more)
fails; without the side_join() of GradBuckets._launch the bucket test fails (at the snapshot of what the collective is given).
"""
import contextlib
import json
import os
import time

import numpy as np
import pytest
import torch

import stream_delay as sd

pytestmark = pytest.mark.gpu


def _need_harness():
    """Every test leans on the harness: where its self-check fails they fail with it (never skip)."""
    ok, text = sd.self_check()
    assert ok, "the delay harness does not work on this machine: " + text


def _beside_main():
    found = sd.independent_streams(1)
    assert found, "no stream of torch's pool runs beside the current stream on this machine"
    return found[0]


def _say(case, **kv):
    print("stream-order {}: {}".format(case, " ".join("{}={}".format(k, ("{:.2f}".format(v) if isinstance(v, float) else v))
                                                         for k, v in kv.items())))


# ------------------------------------------------------------------------------------------------ a. the harness itself
def test_harness_holds_one_stream_and_only_that_one():
    ok, text = sd.self_check()
    cal = sd.calibrate()
    _say("harness", method=cal[0], per_ms=float(cal[1]) if cal[0] == "sleep" else float(cal[2]), check=text.replace(" ", "_"))
    assert ok, text


# ------------------------------------------------------------------------------------------------ the training configurations
@contextlib.contextmanager
def _switches(side, first2d=True, first3d=True, deconv=True):
    """side False: everything on one stream.  side True: every conv unit of every precision, every 3-D layer and the
    transposed convs take the side stream."""
    from boxsegliver_amd import ops
    saved = (ops._Side.enabled, ops._Side.mode, ops.SIDE_WGRAD_FIRST, ops.SIDE_WGRAD3D_FIRST, ops.SIDE_DECONV,
             ops.SIDE_WGRAD3D_VOXELS, ops._Side.stream)
    ops._Side.enabled, ops._Side.mode = bool(side), ("1" if side else "0")
    if side:            # a stream SEEN to run beside the main stream: one that shares its hardware queue cannot be held alone
        ops._Side.stream = _beside_main()
    ops.SIDE_WGRAD_FIRST, ops.SIDE_WGRAD3D_FIRST, ops.SIDE_DECONV = bool(first2d), bool(first3d), bool(deconv)
    ops.SIDE_WGRAD3D_VOXELS = (1 << 30) if side else 0
    try:
        yield
    finally:
        if ops._Side.pending:           # a test that failed half-way: nothing of it stays on the stream that is put back
            ops.side_join()
        (ops._Side.enabled, ops._Side.mode, ops.SIDE_WGRAD_FIRST, ops.SIDE_WGRAD3D_FIRST, ops.SIDE_DECONV,
         ops.SIDE_WGRAD3D_VOXELS, ops._Side.stream) = saved


def _guided_inputs(size, g_ch=1):
    from boxsegliver_amd.data.synthetic import make_batch, make_guide
    images, labels, _ = make_batch(2, size, size, 3, 3, 1234)
    guide = make_guide(labels, g_ch, 1234)
    return {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
            "sp_guide": torch.from_numpy(guide).cuda()}


def _build_unet(dtype="fp32"):
    import test_gpu_unet as t
    args = t.make_args(batch_size=2, im_height=64, im_width=64, compute_dtype=dtype)
    images, labels = t.synth(2, 64, 64, 3, seed=9)
    model, inputs = t.build(args, images, labels)
    return model, inputs, t.YML, args


def _build_gunet(normalizer, g_ch=1, se_drop=False):
    import test_gpu_gunet as t
    if se_drop:         # the SE gate on every modulated unit, dropout on the first unit of every encoder block
        yml = dict(t.YML, context_fc_channels=[32, 16])
        args = t.make_args(normalizer=normalizer, dropout=0.3, use_context=True, use_se=True, side_dropout=0.0,
                           im_height=64, im_width=64)
        model, inputs, _, _, _ = t._setup_variant(args, yml, dict(use_se=True), ctx_len=10, size=64)
    else:
        yml = t.YML
        args = t.make_args(normalizer=normalizer, guide_channel=g_ch, im_height=64, im_width=64)
        model, inputs, _, _, _ = t._setup_variant(args, yml, {}, size=64)
    return model, inputs, yml, args


def _build_zoo(name):
    import yaml
    from pathlib import Path
    import test_gpu_gunet as t
    from boxsegliver_amd import ops
    from boxsegliver_amd.core import models
    zoo = {cls.__name__: cls for cls in models.MODEL_ZOO}
    if name == "LGNet":
        yml = yaml.safe_load((Path(ops.__file__).parent / "NetworksV2" / "LGNet.yml").read_text())
        yml.update(build_metrics=True, build_summaries=False)
    else:
        yml = dict(init_channel_factor=1, num_pool_layers=3, ret_prob=False, ret_pred=True, build_metrics=True,
                   build_summaries=False)
    args = t.make_args(normalizer="batch_norm", use_spatial=True, guide_channel=1, im_height=64, im_width=64)
    inputs = _guided_inputs(64)
    model = zoo[name](args)
    model(inputs, "eval", **yml)
    return model, inputs, yml, args


def _build_unet3d(dtype="fp32"):
    import test_gpu_unet3d as t
    from boxsegliver_amd.NetworksV2.UNet3D import UNet3D
    from boxsegliver_amd.data.synthetic import make_batch_3d
    args = t.make_args(batch_size=1, im_depth=16, im_height=32, im_width=32, learning_rate=1e-3, compute_dtype=dtype)
    images, labels, _ = make_batch_3d(1, 16, 32, 32, 1, 2, 31)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda()}
    model = UNet3D(args)
    model(inputs, "eval", **t.YML)
    return model, inputs, t.YML, args


# name -> (builder, its kwargs, switches of the side run, kinds the side run must reach, exact launches per backward or None)
# UNet: 18 conv units and 4 transposed convs; the first unit has no input gradient (its input is the image), so its filter
# gradient is all there is to do and it stays on the main stream (Conv3x3NormRelu.backward: `ctx.need_dx`): 17 and 4.
CONFIGS = {
    "unet-fp32": (_build_unet, dict(dtype="fp32"), {}, ("conv2d", "deconv"), dict(conv2d=17, deconv=4)),
    "unet-bf16": (_build_unet, dict(dtype="bf16"), {}, ("conv2d", "deconv"), dict(conv2d=17, deconv=4)),
    "unet-bf16c": (_build_unet, dict(dtype="bf16c"), {}, ("conv2d", "deconv"), dict(conv2d=17, deconv=4)),
    "unet-fp32-wgrad-after-dgrad": (_build_unet, dict(dtype="fp32"), dict(first2d=False), ("conv2d", "deconv"),
                                    dict(conv2d=17, deconv=4)),
    "unet-fp32-deconv-on-main": (_build_unet, dict(dtype="fp32"), dict(deconv=False), ("conv2d",), dict(conv2d=17, deconv=0)),
    "gunet-batch-norm": (_build_gunet, dict(normalizer="batch_norm", g_ch=2), {}, ("conv2d", "deconv"), None),
    "gunet-instance-norm": (_build_gunet, dict(normalizer="instance_norm", g_ch=1), {}, ("conv2d", "deconv"), None),
    "gunet-se-dropout": (_build_gunet, dict(normalizer="batch_norm", se_drop=True), {}, ("conv2d", "deconv"), None),
    "lgnet": (_build_zoo, dict(name="LGNet"), {}, ("conv2d", "deconv"), None),
    "interunet": (_build_zoo, dict(name="InterUNet"), {}, ("conv2d",), None),
    "smallunet": (_build_zoo, dict(name="SmallUNet"), {}, ("conv2d",), None),
    "unet3d-fp32": (_build_unet3d, dict(dtype="fp32"), {}, ("conv3d", "deconv"), None),
    "unet3d-fp32-wgrad-after-dgrad": (_build_unet3d, dict(dtype="fp32"), dict(first3d=False), ("conv3d", "deconv"), None),
    "unet3d-bf16c": (_build_unet3d, dict(dtype="bf16c"), {}, ("conv3d", "deconv"), None),
    "unet3d-bf16c-wgrad-after-dgrad": (_build_unet3d, dict(dtype="bf16c"), dict(first3d=False), ("conv3d", "deconv"), None),
}
STEPS = 3
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _REF.clear()
    torch.cuda.empty_cache()


def _snapshot(model):
    return {k: v.clone() for k, v in model.params.flat.items()}


def _train(name, side, steps, side_ms=0.0, main_ms=None, timed=False):
    """`steps` optimiser steps of configuration `name` on a fresh model.  side_ms: hold the side stream (late_side);
    main_ms: {step: ms} hold the main stream right before that step's backward; timed: measure each step's forward +
    backward + optimiser span with the device idle at both ends (the undelayed run only).  Nothing is read back and the
    device is not synchronised between a delayed backward and the optimiser: the comparison happens at the end."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.core.solver import Solver
    builder, kw, sw, _, _ = CONFIGS[name]
    with _switches(side, **(sw if side else {})):
        model, inputs, yml, args = builder(**kw)
        solver = Solver(args)
        out = {"init": _snapshot(model), "loss": [], "grad": [], "spans": []}
        with sd.late_side(ops, side_ms) as counts:
            for s in range(steps):
                span = sd.Span() if timed else contextlib.nullcontext()
                with span:
                    loss = model(inputs, "train", **yml)
                    if main_ms and main_ms.get(s):
                        sd.late_main(main_ms[s])
                    solver(loss, model)
                if timed:
                    out["spans"].append(span.ms)
                out["loss"].append(loss.detach().clone())
                out["grad"].append({k: v.clone() for k, v in model.params.grad.items()})
        out["flat"] = _snapshot(model)
        out["counts"] = dict(counts)
        torch.cuda.synchronize()
    return out


def _reference(name):
    """The single-stream run of `name`, once per module; T = the slowest step after the first (which builds the packs)."""
    if name not in _REF:
        ref = _train(name, False, STEPS, timed=True)
        assert sum(ref["counts"][k] for k in sd.KINDS) == 0, ref["counts"]
        ref["T"] = max(ref["spans"][1:])
        _REF[name] = ref
    return _REF[name]


def _same(ref, got, steps, what):
    for k in ref["init"]:
        assert torch.equal(ref["init"][k], got["init"][k]), (what, "initial variables", k)
    for s in range(steps):
        assert torch.equal(ref["loss"][s], got["loss"][s]), (what, "loss of step", s, float(ref["loss"][s]), float(got["loss"][s]))
        for k in ref["grad"][s]:
            assert torch.equal(ref["grad"][s][k], got["grad"][s][k]), (what, "gradients of step", s, k)


def _check_counts(name, counts, backwards):
    _, _, _, kinds, exact = CONFIGS[name]
    for k in kinds:
        assert counts[k] > 0, ("this configuration quietly stayed on one stream", name, counts)
    if exact:
        for k, n in exact.items():
            assert counts[k] == n * backwards, (name, counts, exact, backwards)


# ------------------------------------------------------------------------------------------------ b. late side stream
@pytest.mark.parametrize("name", list(CONFIGS))
def test_late_side_stream_whole_training_steps(name):
    """Three optimiser steps with the side stream held for D from the first side launch of every backward: the main stream
    finishes backward, reuses the freed dy / x blocks and reaches the optimiser while no filter gradient has run.  The join
    before the optimiser, record_stream, and any in-place write of dy / x / the scratch after the launch are on trial."""
    _need_harness()
    ref = _reference(name)
    d = sd.delay_for(ref["T"])
    got = _train(name, True, STEPS, side_ms=d)
    _say("late-side " + name, T=ref["T"], D=d, **got["counts"])
    _check_counts(name, got["counts"], STEPS)
    assert got["counts"]["holds"] >= STEPS
    _same(ref, got, STEPS, name)
    for k in ref["flat"]:
        assert torch.equal(ref["flat"][k], got["flat"][k]), (name, "variables after the steps", k)


# ------------------------------------------------------------------------------------------------ c. late main stream
@pytest.mark.parametrize("name", list(CONFIGS))
def test_late_main_stream_side_kernels_wait_for_dy(name):
    """The main stream held for D right before the second step's backward (the first step, undelayed, builds the packs): the
    host queues the whole backward while nothing of it runs; a side kernel that does not wait for dy runs at once and reads
    what is not there yet.  side.wait_stream(main) at every launch site is on trial."""
    _need_harness()
    ref = _reference(name)
    d = sd.delay_for(ref["T"])
    got = _train(name, True, 2, main_ms={1: d})
    _say("late-main " + name, T=ref["T"], D=d, **got["counts"])
    _check_counts(name, got["counts"], 2)
    _same(ref, got, 2, name)


# ------------------------------------------------------------------------------------------------ d. a backward that raises
class _Stop(RuntimeError):
    pass


def test_a_backward_that_raised_leaves_no_side_work_unjoined():
    """Under late_side a hook on an early activation (the second encoder level's skip) raises when backward gets there: the
    decoder's and the deep levels' filter gradients are on the held side stream and the engine never runs side_join.  The
    next step (zero_grad -> new_step joins) equals the same step of an undisturbed single-stream run bit for bit."""
    _need_harness()
    from boxsegliver_amd import ops
    from boxsegliver_amd.core.solver import Solver

    def run(side, ms, fail):
        with _switches(side):
            model, inputs, yml, args = _build_unet("fp32")
            solver = Solver(args)
            before = None
            with sd.late_side(ops, ms) as counts:
                loss = model(inputs, "train", **yml)             # both runs: the forward moves the moving statistics
                if fail:
                    def stop(_grad):
                        raise _Stop("stopped on purpose at Encode2")
                    model.layers["Encode2"].register_hook(stop)
                    with pytest.raises(_Stop):
                        solver(loss, model)
                    before = dict(counts)
                    assert ops._Side.pending, "nothing was left on the side stream"
                with (contextlib.nullcontext() if fail else sd.Span()) as span:
                    loss = model(inputs, "train", **yml)
                    solver(loss, model)
                res = (loss.detach().clone(), {k: v.clone() for k, v in model.params.grad.items()}, _snapshot(model))
            torch.cuda.synchronize()
            assert not ops._Side.pending
        return res, before, (None if fail else span.ms)

    ref, _, t = run(False, 0.0, False)
    d = sd.delay_for(t)
    got, before, _ = run(True, d, True)
    _say("raised-backward", T=t, D=d, **before)
    assert before["conv2d"] >= 4 and before["deconv"] >= 1 and before["conv2d"] < 17, before
    assert torch.equal(ref[0], got[0]), (float(ref[0]), float(got[0]))
    for k in ref[1]:
        assert torch.equal(ref[1][k], got[1][k]), ("gradients", k)
    for k in ref[2]:
        assert torch.equal(ref[2][k], got[2][k]), ("variables", k)


# ------------------------------------------------------------------------------------------------ e. data-parallel bucket
def test_late_side_stream_bucket_is_reduced_with_its_filter_gradients():
    """A world of one on RCCL (as test_dp.py::test_rccl_bucketed_allreduce_from_backward_hooks_world1 sets it up, in this
    process).  Under late_side every bucket launched from inside backward must hold its filter gradients.  In a world of
    one the reduction is the identity, so a gradient that lands late would still be in the buffer after finish(): what the
    collective is GIVEN is therefore snapshot on the launching stream right before each all_reduce, and both the snapshots
    and the flat buffer after finish() equal the single-stream gradients."""
    _need_harness()
    import torch.distributed as dist
    import test_dp as t
    from boxsegliver_amd import ops
    from boxsegliver_amd.NetworksV2.UNet import UNet
    from boxsegliver_amd.utils import distribution_utils as du

    def build():
        model = UNet(t._unet_args(2, 1))
        inputs = t._shard(0)
        model(inputs, "eval", **t.YML)
        return model, inputs

    with _switches(False):
        model, inputs = build()
        with sd.Span() as span:
            model.params.zero_grad()
            model(inputs, "train", **t.YML).backward()
        model.params.zero_grad()
        model(inputs, "train", **t.YML).backward()          # the delayed run's second backward (moving statistics differ)
        want = model.params.gbuf.clone()
        torch.cuda.synchronize()
    d = sd.delay_for(span.ms)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(t._free_port())
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert not dist.is_initialized()
    dist.init_process_group("nccl", rank=0, world_size=1)
    real, given = du.dist.all_reduce, []

    def spy(tensor, *a, **k):
        given.append((tensor.storage_offset() - model.params.gbuf.storage_offset(), tensor.clone()))
        return real(tensor, *a, **k)

    try:
        with _switches(True):
            model, inputs = build()
            model.params.zero_grad()
            model(inputs, "train", **t.YML).backward()      # undelayed: builds the packs
            warm = torch.zeros(8, device="cuda")
            dist.all_reduce(warm)                           # RCCL sets itself up in its first call: not inside the delay
            torch.cuda.synchronize()
            strategy = du.DistributionStrategy("mirrored", 1, 0)
            buckets = du.GradBuckets(model.params, strategy, bucket_bytes=1 << 20)
            du.dist.all_reduce = spy
            with sd.late_side(ops, d) as counts:
                model.params.zero_grad()
                buckets.arm()
                model(inputs, "train", **t.YML).backward()
                buckets.finish()
                got = model.params.gbuf.clone()
            du.dist.all_reduce = real
            torch.cuda.synchronize()
            last = buckets.last
            buckets.remove()
    finally:
        du.dist.all_reduce = real
        torch.cuda.synchronize()
        dist.destroy_process_group()
    _say("bucket", T=span.ms, D=d, buckets=last["buckets"], fired_in_backward=last["fired_in_backward"], **counts)
    assert last["buckets"] >= 3 and last["fired_in_backward"] > 0 and counts["conv2d"] > 0
    assert len(given) == last["buckets"]
    for off, snap in given:
        assert torch.equal(snap, want[off:off + snap.numel()]), ("a bucket went out without its filter gradients", off)
    assert torch.equal(got, want)
    assert counts["holds"] >= 2, "no side launch followed a bucket's join"


# ------------------------------------------------------------------------------------------------ j. control on project code
def test_control_a_dropped_join_is_seen():
    """The comparison of test b can fail: with ops.side_join replaced for ONE backward by a function that only clears
    `pending`, the filter gradients cloned on the main stream right after backward are not all the reference's.  Stale
    values only: every address stays inside its allocation.  One run."""
    _need_harness()
    from boxsegliver_amd import ops
    ref = _reference("unet-fp32")
    d = sd.delay_for(ref["T"])
    with _switches(True):
        model, inputs, yml, _ = _build_unet("fp32")
        real = ops.side_join

        def only_clear():
            ops._Side.pending = False

        with sd.late_side(ops, d) as counts:
            loss = model(inputs, "train", **yml)
            model.params.zero_grad()
            ops.side_join = only_clear
            try:
                loss.backward()
                got = {k: v.clone() for k, v in model.params.grad.items()}
            finally:
                torch.cuda.synchronize()
                ops.side_join = real
    assert counts["conv2d"] == 17 and counts["holds"] == 1
    assert torch.equal(ref["loss"][0], loss.detach())
    differ = [k for k in got if not torch.equal(got[k], ref["grad"][0][k])]
    _say("control", T=ref["T"], D=d, buffers_that_differ=",".join(differ))
    assert "reg" in differ, "the filter gradients were all there without a join: the delay did not bite"


# ------------------------------------------------------------------------------------------------ f. volume writer
def _volumes(n_vol, n):
    g = torch.Generator().manual_seed(77)
    return [torch.randint(0, 255, (n,), dtype=torch.uint8, generator=g) for _ in range(n_vol)]


def _write_all(tmp, tag, vols, hdr, shape, copy_ms=0.0, main_ms=0.0):
    """MAX_PENDING + 1 submits, so that the first pinned slot is used twice.  After each submit `flat` is dropped and
    same-sized tensors are allocated and filled on the main stream: without flat.record_stream they land on its memory."""
    from boxsegliver_amd.utils import volume_writer
    w = volume_writer.VolumeWriter()
    w._stream = _beside_main()                               # submit() makes its own only when it has none
    paths, junk = [], []
    try:
        for k, v in enumerate(vols):
            src = v.cuda()
            stale = torch.full_like(src, 0x11)
            torch.cuda.synchronize()
            del stale                                        # flat gets this block: what a copy that ran early would see
            if copy_ms:
                sd.hold(w._stream, copy_ms)
            if main_ms:
                sd.late_main(main_ms)
            flat = src.clone()
            path = tmp / "{}_{}.nii".format(tag, k)
            w.submit(path, hdr, shape, flat)
            del flat
            junk = [torch.full_like(src, 0xEE) for _ in range(3)]
            paths.append(path)
    finally:
        w.close()
    del junk
    return paths


@pytest.mark.parametrize("late", ["copy-stream", "main-stream"])
def test_volume_writer_hand_off(tmp_path, late):
    _need_harness()
    from boxsegliver_amd.data import nii_kits
    from boxsegliver_amd.utils import volume_writer
    shape = (64, 64, 48)
    hdr = nii_kits.header_from_meta(shape[::-1], (2.5, 0.8, 0.8), np.uint8)
    vols = _volumes(volume_writer.MAX_PENDING + 1, int(np.prod(shape)))
    want = []
    for k, v in enumerate(vols):
        p = tmp_path / "want_{}.nii".format(k)
        nii_kits.save_flat(v.numpy(), shape, hdr, p)
        want.append(p.read_bytes())
    t0 = time.perf_counter()
    plain = _write_all(tmp_path, "plain", vols, hdr, shape)
    t = (time.perf_counter() - t0) * 1e3 / len(vols)          # one submit with everything around it
    d = sd.delay_for(t)
    _say("volume-writer " + late, T=t, D=d)
    held = _write_all(tmp_path, "held", vols, hdr, shape, **({"copy_ms": d} if late == "copy-stream" else {"main_ms": d}))
    for k in range(len(vols)):
        assert plain[k].read_bytes() == want[k], ("undelayed", k)
        assert held[k].read_bytes() == want[k], (late, k)


# ------------------------------------------------------------------------------------------------ g. slice store
def test_slice_store_refills_a_staging_buffer_only_after_its_upload(tmp_path):
    """The dataset of test_slice_store_streams_chunks_into_the_resident_store (chunk 5 over 21 slices, mixed filters) with
    the main stream held before the load: both staging buffers are filled and their uploads queued while nothing runs, then
    the host wants to refill the first one.  done[slot].synchronize() is on trial."""
    _need_harness()
    import test_gpu_lits_loader as t
    from boxsegliver_amd.data import lits
    rng = np.random.default_rng(3)
    meta, truth = t._write_dataset(tmp_path, 3, 7, 96, rng, "mixed")
    dev = torch.device("cuda", 0)
    lits.SliceStore(tmp_path, meta, dev, chunk=5, threads=4)              # the files are in the page cache, the pool is warm
    with sd.Span() as span:
        lits.SliceStore(tmp_path, meta, dev, chunk=5, threads=4)
    d = sd.delay_for(span.ms)                                              # all five chunks: more than the two that must fit
    _say("slice-store", T=span.ms, D=d)
    sd.late_main(d)
    store = lits.SliceStore(tmp_path, meta, dev, chunk=5, threads=4)
    im = store.im.cpu().numpy().view(np.uint16)
    lb = store.lb.cpu().numpy()
    for (pid, z), (a, l) in truth.items():
        np.testing.assert_array_equal(im[store.offset[pid] + z], a)
        np.testing.assert_array_equal(lb[store.offset[pid] + z], l)


# ------------------------------------------------------------------------------------------------ h. propagation evaluator
@pytest.mark.parametrize("grow", [False, True])
def test_propagation_loop_reads_its_pinned_tables_after_the_copy(tmp_path, monkeypatch, grow):
    """The device loop of test_gpu_propagation.py (its stand-ins for the network included) with the main stream held for a
    few ms before every guide_components and guide_render: the trace of objects, components and decisions equals the
    undelayed trace.  grow: one slice's prior carries 70 more (identical) entries, so obj_host and obj are reallocated in the
    middle of a case."""
    _need_harness()
    import test_gpu_propagation as t
    from boxsegliver_amd import ops
    from boxsegliver_amd.evaluators import evaluator_liver as evl
    t._nii_dataset(tmp_path, noise=False)
    if grow:
        prior = json.loads((tmp_path / "prior.json").read_text())
        sid = sorted(k for k, v in prior["2"].items() if v and min(v[0]["stddev"]) > 2.0)[1]
        prior["2"][sid].extend([json.loads(json.dumps(prior["2"][sid][0])) for _ in range(70)])
        (tmp_path / "prior.json").write_text(json.dumps(prior))
    monkeypatch.setattr(evl._GuidedLoop, "_forward", t._tumour_where_guided)
    ev = t._evaluator(tmp_path, tmp_path / "run", im_height=64, im_width=64)
    plain, held = [], []
    res_plain = ev.run_g(checkpoint_path=None, trace=plain)
    d = 3.0
    real_c, real_r = ops.guide_components, ops.guide_render

    def late_components(*a, **k):
        sd.late_main(d)
        return real_c(*a, **k)

    def late_render(*a, **k):
        sd.late_main(d)
        return real_r(*a, **k)

    monkeypatch.setattr(ops, "guide_components", late_components)
    monkeypatch.setattr(ops, "guide_render", late_render)
    res_held = ev.run_g(checkpoint_path=None, trace=held)
    most = max(len(x[2]) for x in plain)
    _say("propagation grow={}".format(grow), D=d, slices=len(plain), most_objects=most)
    assert (most > 64) == grow
    assert len(plain) == len(held) > 0
    for a, b in zip(plain, held):
        assert a[:2] == b[:2] and a[4] == b[4] and a[5] == b[5]
        np.testing.assert_array_equal(a[2], b[2])
        assert [(c.root, c.area, c.box, c.peak, c.peak_value) for c in a[3]] == \
            [(c.root, c.area, c.box, c.peak, c.peak_value) for c in b[3]]
        for c, e in zip(a[3], b[3]):
            np.testing.assert_array_equal(c.center, e.center)
            np.testing.assert_array_equal(c.stddev, e.stddev)
    assert any(isinstance(x, int) for tr in plain for x in tr[4])
    assert res_plain == res_held


# ------------------------------------------------------------------------------------------------ i. per-step pinned tables
def test_per_step_tables_belong_to_their_own_upload():
    """Two consecutive uploads from fresh pinned memory with the main stream held: the first pinned block is freed by the
    host before its copy has run; the second upload must not get it."""
    _need_harness()
    import argparse
    from boxsegliver_amd.data import lits
    rng = np.random.default_rng(12)
    h = w = 48
    config = argparse.Namespace(im_height=h, im_width=w)
    tab = torch.from_numpy(np.array([[0, 0, 0, 0, h, w, 0, 0], [0, 0, 2, 3, 30, 40, 1, 0]], np.int32)).cuda()
    ptr = np.array([0, 3, 5], np.int32)
    objs = [np.concatenate([rng.uniform(0, 40, (5, 2)), rng.uniform(2, 9, (5, 2))], 1).astype(np.float32) for _ in range(2)]
    table = torch.from_numpy(rng.random((7, 200)).astype(np.float32)).cuda()
    ctab = np.zeros((8, 10), np.int32)
    ctab[:, 3] = [2, 5, 2, -1, 0, 6, 2, 3]
    ctab_d = torch.from_numpy(ctab).cuda()
    takes = [np.array([1, 1, 1, 1, 0, 1, 1, 0], np.int32), np.array([0, 1, 0, 1, 1, 0, 1, 1], np.int32)]

    def both():
        sp = [lits.render_guide(tab, ptr, o, config, 1, (h, w)) for o in objs]
        cx = [lits.guides(ctab_d, tk, None, None, None, table, config, 3, (h, w))[1] for tk in takes]
        return sp + cx

    with sd.Span() as span:
        want = both()
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[2], want[3])
    d = sd.delay_for(span.ms)
    _say("pinned-tables", T=span.ms, D=d)
    sd.late_main(d)
    got = both()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), k
