"""The measurement of the in-plane rotated LiTS 3-D batches in DESIGN.md 7.3.9, taken in one process on one MI355X: the device
time, between device events, of one `liver_3d` training batch at 10 x 256 x 256 batch 4 and at one 96^3 patch (the store, the
tables and the clicks of tools/measure_lits3d_clicks.py: zoom 1.25 on 512 x 512 slices)
  * unguided (`unetk_lits_pick_voxel` + the patch entry) and guided (+ `unetk_lits3d_clicks` + the guide entry),
  * with --random_rotate 0 (the plain entries), with the _rot entries on the same table (columns 13 / 14 zero: the rows that are
    not rotated must not get slower) and with --random_rotate 30 --rotate_prob 1 (every row turned by an angle from U(-30, 30)),
and the rotated batches' extra time as a share of the UNet3D training step at that shape (the README's measured step).
Medians of 10.
Usage: python tools/measure_lits3d_rotate.py [out.json]   (needs a GPU)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure_lits3d_clicks as base  # noqa: E402
from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.data import lits, lits3d  # noqa: E402

OUT = {}
DEG = 30.0
STEP_MS = {(10, 256, 256): 49.6, (96, 96, 96): 18.9}      # README: one UNet3D training step at these shapes


def _rotated(tab, deg):
    """The table with every row turned by an angle from U(-deg, deg), as PatchSampler.table writes it."""
    t = tab.cpu().numpy().copy()
    rad = np.deg2rad(np.random.default_rng(2).uniform(-deg, deg, len(t)))
    t[:, lits3d.COL_SIN] = np.sin(rad).astype(np.float32).view(np.int32)
    t[:, lits3d.COL_COS] = np.cos(rad).astype(np.float32).view(np.int32)
    return torch.from_numpy(t).to(tab.device)


def _plain(im, lb, tab, shape, status, rotate):
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    return ops.lits_patch3d(im, lb, tab, shape, True, 2, lits.IM_SCALE, lits.LB_SCALE, rotate=rotate)


def _batch(im, lb, tab, ctab, shape, status, rotate):
    images, labels = _plain(im, lb, tab, shape, status, rotate)
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, 2, lits3d.CLICKS, lits.LB_SCALE)
    return images, labels, ops.click_guide3d(tab, pts, cnt, shape, base.SRC, 2, base.STDDEV, rotate=rotate)


def measure(im, lb, bs, shape):
    dev = im.device
    tab, ctab = base._tables(dev, bs, shape)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    variants = (("deg0_plain_entries", tab, False), ("deg0_rot_entries", tab, True), ("deg30_rot_entries", _rotated(tab, DEG), True))
    out = {"shape": dict(batch=bs, dhw=shape, crop=(int(shape[1] * base.ZOOM), int(shape[2] * base.ZOOM)), slices=base.SRC)}
    for name, t, rotate in variants:
        out[name] = dict(unguided=base._event_ms(lambda: _plain(im, lb, t, shape, status, rotate)),
                         guided=base._event_ms(lambda: _batch(im, lb, t, ctab, shape, status, rotate)))
        print(shape, name, out[name], flush=True)
    assert int(status.item()) == 0
    a, b = _batch(im, lb, tab, ctab, shape, status, False), _batch(im, lb, tab, ctab, shape, status, True)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))      # zero columns: the same batch
    kernels = base._by_kernel(lambda: _batch(im, lb, variants[2][1], ctab, shape, status, True))
    out["deg30_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    for kind in ("unguided", "guided"):
        extra = out["deg30_rot_entries"][kind]["ms_median"] - out["deg0_plain_entries"][kind]["ms_median"]
        out["extra_ms_" + kind] = extra
        out["extra_share_of_step_" + kind] = extra / STEP_MS[tuple(shape)]
    print(shape, "rotation costs", {k: v for k, v in out.items() if k.startswith("extra")}, flush=True)
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
