"""The measurement of the z-resampled LiTS 3-D batches in DESIGN.md 7.3.17, taken in one process on one MI355X: the device time,
between device events, of
  * one unguided `liver_3d` training batch (`unetk_lits_pick_voxel` + the patch entry) at 10 x 256 x 256 batch 4 and at one 96^3
    patch (the store and the tables of tools/measure_lits3d_clicks.py: zoom 1.25 on 512 x 512 slices) -- without --z_spacing (the
    plain entry), and through `unetk_lits_patch3d_z` with every crop depth D (the rows must come out bit for bit and should cost
    what the plain batch costs), with every crop depth 2 D and with every crop depth D / 2;
  * `unetk_eval3d_accumulate_z` beside `unetk_eval3d_accumulate` on four 10 x 256 x 256 windows (the case and the windows of
    tools/measure_eval3d_weighted.py), with every crop depth D, 2 D and D / 2,
and each flagged batch's extra time as a share of the UNet3D training step at that shape (the README's measured step).
Medians of 10.
Usage: python tools/measure_lits3d_zspace.py [out.json]   (needs a GPU)"""
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
STEP_MS = {(10, 256, 256): 49.6, (96, 96, 96): 18.9}      # README: one UNet3D training step at these shapes
CASE, WINDOW, C = (75, 512, 512), (10, 256, 256), 3        # tools/measure_eval3d_weighted.py


def _batch(im, lb, tab, shape, status, zcrop=None, zmax=0):
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    return ops.lits_patch3d(im, lb, tab, shape, True, 2, lits.IM_SCALE, lits.LB_SCALE, zcrop=zcrop, zcrop_max=zmax)


def measure_batch(im, lb, bs, shape):
    dev = im.device
    tab, _ = base._tables(dev, bs, shape)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d = shape[0]
    out = {"shape": dict(batch=bs, dhw=shape, crop=(int(shape[1] * base.ZOOM), int(shape[2] * base.ZOOM)), slices=base.SRC)}
    out["flagless"] = base._event_ms(lambda: _batch(im, lb, tab, shape, status))
    for name, cd in (("cd_eq_D", d), ("cd_2D", 2 * d), ("cd_half_D", d // 2)):
        zc = torch.full((bs,), cd, dtype=torch.int32, device=dev)
        out[name] = dict(cd=cd, **base._event_ms(lambda: _batch(im, lb, tab, shape, status, zc, cd)))
        out[name]["extra_ms"] = out[name]["ms_median"] - out["flagless"]["ms_median"]
        out[name]["extra_share_of_step"] = out[name]["extra_ms"] / STEP_MS[tuple(shape)]
        kernels = base._by_kernel(lambda: _batch(im, lb, tab, shape, status, zc, cd))
        out[name]["kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
        print(shape, name, {k: v for k, v in out[name].items() if k != "kernels_ms"}, flush=True)
        print(shape, name, "kernels", out[name]["kernels_ms"], flush=True)
    print(shape, "flagless", out["flagless"], flush=True)
    assert int(status.item()) == 0
    zc = torch.full((bs,), d, dtype=torch.int32, device=dev)
    a, b = _batch(im, lb, tab, shape, status), _batch(im, lb, tab, shape, status, zc, d)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))      # cd == D: the same batch
    return out


def measure_accumulate(dev):
    slices = torch.zeros(CASE, dtype=torch.int16, device=dev)
    case = {"PID": 0, "size": list(CASE)}

    class _Store(object):
        im, offset = np.zeros((0,) + CASE[1:], np.uint16), {0: 0}
    probs = torch.softmax(torch.randn((4,) + WINDOW + (C,), device=dev), dim=-1).contiguous()
    acc = torch.zeros(CASE + (C,), dtype=torch.float32, device=dev)
    cnt = torch.zeros(CASE, dtype=torch.int32, device=dev)
    out = {}
    for name, cd in (("plain", None), ("cd_eq_D", WINDOW[0]), ("cd_2D", 2 * WINDOW[0]), ("cd_half_D", WINDOW[0] // 2)):
        depth = WINDOW[0] if cd is None else cd
        tab = next(lits3d.eval_tables(case, _Store, WINDOW, 0.5, [(0, 0, 0)], 4, box=(0, depth, 0, 432, 0, 512), cd=cd))
        assert len(tab) == 4
        box = lits3d.table_box(tab, WINDOW, CASE[0], CASE[1:], cd=cd)
        assert box == (0, depth, 0, 432, 0, 512), box
        dtab = torch.from_numpy(tab).to(dev)
        kw = {} if cd is None else dict(zcrop=torch.full((4,), cd, dtype=torch.int32, device=dev), zcrop_max=cd)
        nvox = (box[1] - box[0]) * (box[3] - box[2]) * (box[5] - box[4])
        out[name] = dict(cd=cd, voxels=nvox, **base._event_ms(
            lambda: ops.eval3d_accumulate(probs, dtab, WINDOW, 0, CASE[0], box, acc, cnt, slices, host_tab=tab, **kw)))
        out[name]["ns_per_voxel"] = out[name]["ms_median"] * 1e6 / nvox
        print("accumulate", name, out[name], flush=True)
    out["ratio_cd_eq_D"] = out["cd_eq_D"]["ms_median"] / out["plain"]["ms_median"]
    return out


def main():
    dev = torch.device("cuda")
    im, lb = base._store(dev)
    for bs, shape in base.SHAPES:
        OUT["x".join(str(v) for v in shape) + "_bs{}".format(bs)] = measure_batch(im, lb, bs, shape)
        torch.cuda.empty_cache()
    del im, lb
    OUT["accumulate"] = measure_accumulate(dev)
    print("accumulate_z / accumulate at cd == D:", OUT["accumulate"]["ratio_cd_eq_D"], flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no device: nothing to measure")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
