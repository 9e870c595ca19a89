"""The measurement of the click-guided LiTS 3-D batches in DESIGN.md 7.3.6, taken in one process on one MI355X: the device
time of one `liver_3d --use_spatial` training batch -- `unetk_lits_pick_voxel` + `unetk_lits_patch3d` + `unetk_lits3d_clicks` +
`unetk_click_guide3d`, between device events -- at 10 x 256 x 256 batch 4 and at one 96^3 patch, zoom 1.25 on 512 x 512
slices, every sample asking for four clicks of each kind; the unguided batch (pick + patch) at the same tables; the split by
kernel (the library's per-dispatch events); and beside it one UNet3D training step (forward, backward, Adam) at that shape on
those batches.  Medians of 10.
Usage: python tools/measure_lits3d_clicks.py [out.json]   (needs a GPU)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.core import models, solver  # noqa: E402
from boxsegliver_amd.data import lits, lits3d, lits_inter  # noqa: E402
from boxsegliver_amd.entry import main as entry  # noqa: E402

OUT = {}
SRC, DEPTH, ZOOM = (512, 512), 128, 1.25
SHAPES = ((4, (10, 256, 256)), (1, (96, 96, 96)))
STDDEV = (1.0, 3.0, 3.0)
REPS = 10


def _store(dev):
    """A LiTS-sized synthetic case: noise over a body ellipse, a liver ellipse (label 1) that swells and shrinks through the
    slices with tumour discs (label 2) on every slice, so every patch has an object whose erosion is non-empty on many
    slices and a band the crop cuts."""
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(SRC[0]), np.arange(SRC[1]), indexing="ij")
    lab = np.zeros((DEPTH,) + SRC, np.uint8)
    for z in range(DEPTH):
        s = 0.6 + 0.4 * np.sin(np.pi * (z + 0.5) / DEPTH)
        lab[z][((yy - 260) / (110. * s)) ** 2 + ((xx - 200) / (140. * s)) ** 2 <= 1] = 1
        for cy, cx, r in ((230, 180, 22), (300, 260, 14), (250, 120, 7)):
            lab[z][(yy - cy) ** 2 + (xx - cx - z % 7) ** 2 <= r * r] = 2
    body = ((yy - 256) / 200.) ** 2 + ((xx - 256) / 240.) ** 2 <= 1
    im = np.where(body, rng.normal(240, 35, (DEPTH,) + SRC).astype(np.float32) + 70 * (lab > 0) - 50 * (lab == 2), 0)
    im = (np.clip(im, 0, 450) * lits.IM_SCALE).astype(np.uint16)
    return torch.from_numpy(im.view(np.int16)).to(dev), torch.from_numpy(lab * np.uint8(lits.LB_SCALE)).to(dev)


def _tables(dev, bs, shape):
    """One batch as PatchSampler.table lays it out: the first half of the samples (at least one) forced onto a tumour voxel."""
    rng = np.random.default_rng(1)
    tab = np.zeros((bs, 16), np.int32)
    tab[:, 1] = DEPTH
    tab[:, 2] = rng.integers(shape[0] // 2, DEPTH - shape[0] // 2, bs)
    tab[:, 3], tab[:, 4] = rng.integers(150, 360, bs), rng.integers(100, 330, bs)
    tab[:, 5], tab[:, 6] = int(shape[1] * ZOOM), int(shape[2] * ZOOM)
    tab[:, 7:10] = rng.integers(0, 2, (bs, 3))
    tab[:, 10] = rng.uniform(0.7, 1.5, bs).astype(np.float32).view(np.int32)
    force = max(bs // 2, 1)
    tab[:force, 11], tab[:force, 12] = 1, rng.integers(0, 1000, force)
    clicks = lits_inter.draw_click_tab(rng, bs)
    clicks[:, 0], clicks[:, 1] = 4, 4                                        # the most clicks a sample can ask for
    clicks[:, 2] = np.where(np.arange(bs) % 2 == 0, 3, 1)                    # sample 0 takes the whole-patch arg-max
    return torch.from_numpy(tab).to(dev), torch.from_numpy(clicks.view(np.int32)).to(dev)


def _plain(im, lb, tab, shape, status):
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    return ops.lits_patch3d(im, lb, tab, shape, True, 2, lits.IM_SCALE, lits.LB_SCALE)


def _batch(im, lb, tab, ctab, shape, status):
    images, labels = _plain(im, lb, tab, shape, status)
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, 2, lits3d.CLICKS, lits.LB_SCALE)
    guide = ops.click_guide3d(tab, pts, cnt, shape, SRC, 2, STDDEV)
    return images, labels, guide, cnt


def _event_ms(fn):
    for _ in range(3):
        fn()
    per = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b))
    return dict(ms_median=statistics.median(per), ms_min=min(per), ms_max=max(per), reps=len(per))


def _by_kernel(fn):
    """Median over REPS calls of the time of every kernel the library dispatches in fn(), summed by kernel name."""
    torch.cuda.synchronize()
    per = {}
    for _ in range(REPS):
        ops.profile_begin(64)
        ops.profile_on([])
        fn()
        torch.cuda.synchronize()
        ms, names = ops.profile_read()
        ops.profile_on(None)
        once = {}
        for t, name in zip(ms, names):
            once[name] = once.get(name, 0.0) + t
        for name, t in once.items():
            per.setdefault(name, []).append(t)
    return {name: statistics.median(v) for name, v in per.items()}


def measure(im, lb, bs, shape):
    dev = im.device
    out = {}
    tab, ctab = _tables(dev, bs, shape)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    images, labels, guide, cnt = _batch(im, lb, tab, ctab, shape, status)
    assert int(status.item()) == 0 and int(labels.max()) == 2 and int(cnt.min()) >= 1
    out["shape"] = dict(batch=bs, dhw=shape, crop=(int(shape[1] * ZOOM), int(shape[2] * ZOOM)), slices=SRC,
                        clicks=cnt.cpu().numpy().tolist())
    out["unguided_batch_events"] = _event_ms(lambda: _plain(im, lb, tab, shape, status))
    out["batch_events"] = _event_ms(lambda: _batch(im, lb, tab, ctab, shape, status))
    kernels = _by_kernel(lambda: _batch(im, lb, tab, ctab, shape, status))
    out["batch_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    out["batch_kernels_sum_ms"] = sum(kernels.values())
    print(shape, "unguided", out["unguided_batch_events"], "guided", out["batch_events"], flush=True)
    print(shape, "kernels", out["batch_kernels_ms"], "sum", out["batch_kernels_sum_ms"], flush=True)

    argv = ("liver_3d --mode train --tag measure --model UNet3D --classes Liver Tumor --im_depth {} --im_height {} --im_width {} "
            "--im_channel 1 --batch_size {} --normalizer instance_norm --loss_weight_type numerical --loss_numeric_w 1 1 3 "
            "--use_spatial --local_enhance").format(shape[0], shape[1], shape[2], bs).split()
    args, _, _ = entry.get_arguments(argv)
    params = {"args": args}
    params.update(models.get_model_params(args, build_metrics=True))
    params.update(solver.get_solver_params(args))
    feats = {"images": images, "sp_guide": guide}

    def step():
        spec = models.model_fn(feats, labels, "train", params)
        return spec.loss
    out["unet3d_step_events"] = _event_ms(step)
    out["batch_share_of_step"] = out["batch_events"]["ms_median"] / out["unet3d_step_events"]["ms_median"]
    out["guide_share_of_step"] = (out["batch_events"]["ms_median"] - out["unguided_batch_events"]["ms_median"]) / \
        out["unet3d_step_events"]["ms_median"]
    print(shape, "UNet3D step", out["unet3d_step_events"], "batch / step = {:.4f}, clicks + guide / step = {:.4f}".format(
        out["batch_share_of_step"], out["guide_share_of_step"]), flush=True)
    return out


def main():
    dev = torch.device("cuda")
    im, lb = _store(dev)
    for bs, shape in SHAPES:
        OUT["x".join(str(v) for v in shape) + "_bs{}".format(bs)] = measure(im, lb, bs, shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no device: nothing to measure")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
