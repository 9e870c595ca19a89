"""The measurement of the 3-D boundary weights in DESIGN.md 7.3.12, taken in one process on one MI355X, at 10 x 256 x 256 batch
4 and at one 96^3 patch (the store and the tables of tools/measure_lits3d_clicks.py: liver and tumour labels, zoom 1.25 on
512 x 512 slices):
  * the kernel sequence of `unetk_boundary_weights3d` alone on the batch's labels, between device events, at --boundary_z_scale 1
    and 3, and its split by kernel (the library's per-dispatch events),
  * one UNet3D training step (forward, backward, Adam) on that batch with --loss_weight_type none and with --loss_weight_type
    boundary, and the difference as a share of the step without the flag.
Medians of 10.
Usage: python tools/measure_boundary3d.py [out.json]   (needs a GPU)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import measure_lits3d_clicks as base  # noqa: E402
from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.core import models, solver  # noqa: E402
from boxsegliver_amd.entry import main as entry  # noqa: E402

OUT = {}


def _step_fn(images, labels, bs, shape, w_type):
    argv = ("liver_3d --mode train --tag measure --model UNet3D --classes Liver Tumor --im_depth {} --im_height {} --im_width {} "
            "--im_channel 1 --batch_size {} --normalizer instance_norm --loss_weight_type {}").format(
                shape[0], shape[1], shape[2], bs, w_type).split()
    args, _, _ = entry.get_arguments(argv)
    params = {"args": args}
    params.update(models.get_model_params(args, build_metrics=True))
    params.update(solver.get_solver_params(args))
    feats = {"images": images}
    return lambda: models.model_fn(feats, labels, "train", params).loss


def measure(im, lb, bs, shape):
    tab, _ = base._tables(im.device, bs, shape)
    status = torch.zeros(1, dtype=torch.int32, device=im.device)
    images, labels = base._plain(im, lb, tab, shape, status)
    assert int(status.item()) == 0 and int(labels.max()) == 2
    out = {"shape": dict(batch=bs, dhw=shape)}
    wmap, d2 = ops.boundary_weights3d(labels, 1, want_d2=True)
    out["ring_voxels_share"] = float((d2 == 0).float().mean())
    out["ring_free_samples"] = int((d2.reshape(bs, -1)[:, 0] < 0).sum())
    out["largest_distance"] = float(d2.max()) ** 0.5
    for k in (1, 3):
        out["map_events_k{}".format(k)] = base._event_ms(lambda: ops.boundary_weights3d(labels, k))
    kernels = base._by_kernel(lambda: ops.boundary_weights3d(labels, 1))
    out["map_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    out["map_kernels_sum_ms"] = sum(kernels.values())
    print(shape, {k: v for k, v in out.items() if k != "map_kernels_ms"}, flush=True)
    print(shape, "kernels", out["map_kernels_ms"], flush=True)
    for w_type in ("none", "boundary"):
        out["unet3d_step_" + w_type] = base._event_ms(_step_fn(images, labels, bs, shape, w_type))
        torch.cuda.empty_cache()
    plain = out["unet3d_step_none"]["ms_median"]
    out["extra_ms"] = out["unet3d_step_boundary"]["ms_median"] - plain
    out["extra_share_of_step"] = out["extra_ms"] / plain
    out["map_share_of_step"] = out["map_events_k1"]["ms_median"] / plain
    print(shape, "UNet3D step", out["unet3d_step_none"], "with boundary", out["unet3d_step_boundary"],
          "map / step = {:.4f}, (boundary - none) / none = {:.4f}".format(out["map_share_of_step"], out["extra_share_of_step"]),
          flush=True)
    return out


def main():
    dev = torch.device("cuda")
    im, lb = base._store(dev)
    for bs, shape in base.SHAPES:
        OUT["x".join(str(v) for v in shape) + "_bs{}".format(bs)] = measure(im, lb, bs, shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no device: nothing to measure")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
