"""The measurement of the elastically deformed LiTS 3-D batches in DESIGN.md 7.3.10, taken in one process on one MI355X: the
device time, between device events, of one `liver_3d` training batch at 10 x 256 x 256 batch 4 and at one 96^3 patch (the store,
the tables and the clicks of tools/measure_lits3d_clicks.py: zoom 1.25 on 512 x 512 slices)
  * unguided (`unetk_lits_pick_voxel` + the patch entry) and guided (+ `unetk_lits3d_clicks` + the guide entry),
  * without --random_deform (the plain entries), with the _warp entries on the same table (columns 13 .. 15 zero: the rows that
    are not deformed pay the launches of kernels that return at once) and with --random_deform at the cap, --deform_grid 4,
    --deform_prob 1 (every row deformed),
and the deformed batches' extra time as a share of the UNet3D training step at that shape (the README's measured step).
Medians of 10.
Usage: python tools/measure_lits3d_deform.py [out.json]   (needs a GPU)"""
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
GRID = 4
STEP_MS = {(10, 256, 256): 49.6, (96, 96, 96): 18.9}      # README: one UNet3D training step at these shapes


def _deformed(tab):
    """The table with every row deformed, as PatchSampler.table writes it."""
    t = tab.cpu().numpy().copy()
    t[:, lits3d.COL_WARP] = 1
    return torch.from_numpy(t).to(tab.device)


def _lattices(dev, bs, shape):
    """Control displacements at the cap, as PatchSampler.draw_deform draws them."""
    px = lits3d.deform_cap(shape[1:], GRID)
    ctl = np.random.default_rng(3).uniform(-px, px, (bs, 2, GRID + 3, GRID + 3)).astype(np.float32)
    return torch.from_numpy(ctl).to(dev), px


def _plain(im, lb, tab, shape, status, warp):
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    return ops.lits_patch3d(im, lb, tab, shape, True, 2, lits.IM_SCALE, lits.LB_SCALE, warp=warp, grid=GRID)


def _batch(im, lb, tab, ctab, shape, status, warp):
    images, labels = _plain(im, lb, tab, shape, status, warp)
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, 2, lits3d.CLICKS, lits.LB_SCALE)
    return images, labels, ops.click_guide3d(tab, pts, cnt, shape, base.SRC, 2, base.STDDEV, warp=warp, grid=GRID)


def measure(im, lb, bs, shape):
    dev = im.device
    tab, ctab = base._tables(dev, bs, shape)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    warp, px = _lattices(dev, bs, shape)
    variants = (("off_plain_entries", tab, None), ("off_warp_entries", tab, warp), ("cap_warp_entries", _deformed(tab), warp))
    out = {"shape": dict(batch=bs, dhw=shape, crop=(int(shape[1] * base.ZOOM), int(shape[2] * base.ZOOM)), slices=base.SRC,
                         grid=GRID, px=px)}
    for name, t, w in variants:
        out[name] = dict(unguided=base._event_ms(lambda: _plain(im, lb, t, shape, status, w)),
                         guided=base._event_ms(lambda: _batch(im, lb, t, ctab, shape, status, w)))
        print(shape, name, out[name], flush=True)
    assert int(status.item()) == 0
    a, b = _batch(im, lb, tab, ctab, shape, status, None), _batch(im, lb, tab, ctab, shape, status, warp)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))      # zero columns: the same batch
    c = _batch(im, lb, variants[2][1], ctab, shape, status, warp)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2]) and bool(torch.isfinite(c[0]).all())
    kernels = base._by_kernel(lambda: _batch(im, lb, variants[2][1], ctab, shape, status, warp))
    out["cap_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    for kind in ("unguided", "guided"):
        for name in ("off_warp_entries", "cap_warp_entries"):
            extra = out[name][kind]["ms_median"] - out["off_plain_entries"][kind]["ms_median"]
            out["extra_ms_{}_{}".format(name, kind)] = extra
            out["extra_share_of_step_{}_{}".format(name, kind)] = extra / STEP_MS[tuple(shape)]
    print(shape, "deformation costs", {k: v for k, v in out.items() if k.startswith("extra")}, flush=True)
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
