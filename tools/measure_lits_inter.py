"""The measurement of the click-guided LiTS batches in DESIGN.md 7.3.5, taken in one process on one MI355X: the device
time of one `liver_inter` training batch -- `unetk_lits_pick_voxel` + `unetk_lits_inter_batch` + `unetk_lits_clicks` +
`unetk_click_guide`, between device events -- at batch 8, 256 x 256 x 3, zoom 1.25 (320 x 320 crops of 512 x 512 slices),
its split by kernel (the library's per-dispatch events), and beside it one `UNetInter` training step (forward, backward,
Adam) at that shape on those batches.  Medians of 10.
Usage: python tools/measure_lits_inter.py [out.json]   (needs a GPU)"""
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
from boxsegliver_amd.data import lits, lits_inter  # noqa: E402
from boxsegliver_amd.entry import main as entry  # noqa: E402

OUT = {}
BS, SHAPE, SRC, DEPTH, ZOOM = 8, (3, 256, 256), (512, 512), 64, 1.25
REPS = 10


def _store(dev):
    """A LiTS-sized synthetic case: noise over a body ellipse, a liver ellipse (label 1) with tumour discs (label 2) on every
    slice, so every sample has an object whose erosion is non-empty and a band the crop cuts."""
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(SRC[0]), np.arange(SRC[1]), indexing="ij")
    lab = np.zeros(SRC, np.uint8)
    lab[((yy - 260) / 110.) ** 2 + ((xx - 200) / 140.) ** 2 <= 1] = 1
    for cy, cx, r in ((230, 180, 22), (300, 260, 14), (250, 120, 7)):
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 2
    body = ((yy - 256) / 200.) ** 2 + ((xx - 256) / 240.) ** 2 <= 1
    im = np.where(body, rng.normal(240, 35, (DEPTH,) + SRC) + 70 * (lab > 0) - 50 * (lab == 2), 0)
    im = (np.clip(im, 0, 450) * lits.IM_SCALE).astype(np.uint16)
    lb = np.broadcast_to(lab * lits.LB_SCALE, (DEPTH,) + SRC).astype(np.uint8)
    return torch.from_numpy(im.view(np.int16)).to(dev), torch.from_numpy(np.ascontiguousarray(lb)).to(dev)


def _tables(dev):
    """One batch as PatchSampler.table lays it out: half the samples forced onto an object pixel, crops 320 x 320."""
    rng = np.random.default_rng(1)
    tab = np.zeros((BS, 16), np.int32)
    tab[:, 1] = DEPTH
    tab[:, 2] = rng.integers(1, DEPTH - 1, BS)
    tab[:, 3], tab[:, 4] = rng.integers(150, 360, BS), rng.integers(100, 330, BS)
    tab[:, 5], tab[:, 6] = int(SHAPE[1] * ZOOM), int(SHAPE[2] * ZOOM)
    tab[:, 7:9] = rng.integers(0, 2, (BS, 2))
    tab[:, 10] = rng.uniform(0.7, 1.5, BS).astype(np.float32).view(np.int32)
    tab[:BS // 2, 11], tab[:BS // 2, 12] = 1, rng.integers(0, 1000, BS // 2)
    clicks = lits_inter.draw_click_tab(rng, BS)
    clicks[:, 0], clicks[:, 1] = 4, 4                                        # the most clicks a sample can ask for
    return torch.from_numpy(tab).to(dev), torch.from_numpy(clicks.view(np.int32)).to(dev)


def _batch(im, lb, tab, ctab, status):
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    images, labels = ops.lits_inter_batch(im, lb, tab, SHAPE, True, status, 2, 0.1, 7, lits.IM_SCALE, lits.LB_SCALE)
    pts, cnt = ops.lits_clicks(lb, tab, ctab, status, 2, lits_inter.CLICKS, lits.LB_SCALE)
    guide = ops.click_guide(tab, pts, cnt, SHAPE[1:], SRC, 2, 5.0)
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


def main():
    dev = torch.device("cuda")
    im, lb = _store(dev)
    tab, ctab = _tables(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    images, labels, guide, cnt = _batch(im, lb, tab, ctab, status)
    assert int(status.item()) == 0 and int(labels.max()) == 1 and int(cnt.min()) >= 1
    OUT["shape"] = dict(batch=BS, hwc=SHAPE[1:] + SHAPE[:1], crop=(int(SHAPE[1] * ZOOM), int(SHAPE[2] * ZOOM)), slices=SRC,
                        clicks=cnt.cpu().numpy().tolist())
    OUT["batch_events"] = _event_ms(lambda: _batch(im, lb, tab, ctab, status))
    kernels = _by_kernel(lambda: _batch(im, lb, tab, ctab, status))
    OUT["batch_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    OUT["batch_kernels_sum_ms"] = sum(kernels.values())
    print("batch", OUT["batch_events"], flush=True)
    print("kernels", OUT["batch_kernels_ms"], "sum", OUT["batch_kernels_sum_ms"], flush=True)

    argv = ("liver_inter --mode train --tag measure --model UNetInter --classes Tumor --im_height {} --im_width {} --im_channel {} "
            "--batch_size {} --normalizer instance_norm --loss_weight_type numerical --loss_numeric_w 1 1 --use_spatial "
            "--local_enhance --stddev 5.").format(SHAPE[1], SHAPE[2], SHAPE[0], BS).split()
    args, _, _ = entry.get_arguments(argv, guided=True)
    params = {"args": args}
    params.update(models.get_model_params(args, build_metrics=True))
    params.update(solver.get_solver_params(args))
    feats = {"images": images, "sp_guide": guide}

    def step():
        spec = models.model_fn(feats, labels, "train", params)
        return spec.loss
    OUT["unetinter_step_events"] = _event_ms(step)
    OUT["batch_share_of_step"] = OUT["batch_events"]["ms_median"] / OUT["unetinter_step_events"]["ms_median"]
    print("UNetInter step", OUT["unetinter_step_events"], "batch / step = {:.4f}".format(OUT["batch_share_of_step"]), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        print("no device: nothing to measure")
        sys.exit(0)
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
