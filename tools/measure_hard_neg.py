"""The measurement of hard-negative training in DESIGN.md 7.3.16, taken in one process on one MI355X, between device events:
  * `unetk_fp_mask3d` on a synthetic 450 x 512 x 512 case (a liver-sized labelled object, a prediction of it that is shifted
    by a few voxels, and a few thousand scattered false alarms of 1 .. 729 voxels);
  * one guided `liver_3d` training batch at 10 x 256 x 256 batch 4 and at one 96^3 patch (the store, the tables and the clicks
    of tools/measure_lits3d_clicks.py) WITH --hard_neg_patches and --hard_neg_clicks (one row centred on a false positive:
    two `unetk_lits_pick_voxel_rows` calls, `unetk_lits_patch3d`, `unetk_lits3d_clicks_neg`, `unetk_click_guide3d`) and with
    NEITHER flag, in the same run; the split by kernel of the flagged batch; and one UNet3D training step at that shape
    beside it, of which the flagged batch is stated as a share.
Medians of 10.
Usage: python tools/measure_hard_neg.py [out.json]   (needs a GPU)"""
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
from boxsegliver_amd.core import models, solver  # noqa: E402
from boxsegliver_amd.data import lits, lits3d  # noqa: E402
from boxsegliver_amd.entry import main as entry  # noqa: E402

OUT = {}
MINE_DEPTH = 450


def _neg_plane(lb):
    """False alarms on the store of measure_lits3d_clicks: on every slice a disc of radius 14 outside the liver and one of
    radius 9 inside it (the label does not matter to the clicks), in the label plane's encoding."""
    yy, xx = np.meshgrid(np.arange(base.SRC[0]), np.arange(base.SRC[1]), indexing="ij")
    neg = np.zeros((base.DEPTH,) + base.SRC, np.uint8)
    for z in range(base.DEPTH):
        neg[z][(yy - 150) ** 2 + (xx - 380 - z % 5) ** 2 <= 14 * 14] = 1
        neg[z][(yy - 300) ** 2 + (xx - 170 + z % 3) ** 2 <= 9 * 9] = 1
    return torch.from_numpy(neg * np.uint8(lits.LB_SCALE)).to(lb.device), neg.sum(axis=(1, 2))


def _flagged(im, lb, neg, tab, ctab, shape, status):
    ops.lits_pick_voxel_rows(lb, tab, lits3d.FORCED_LABEL, status, 2, lits.LB_SCALE)
    ops.lits_pick_voxel_rows(neg, tab, lits3d.FORCED_NEG, status, 1, lits.LB_SCALE)
    images, labels = ops.lits_patch3d(im, lb, tab, shape, True, 2, lits.IM_SCALE, lits.LB_SCALE)
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, 2, lits3d.CLICKS, lits.LB_SCALE, neg_slices=neg)
    return images, labels, ops.click_guide3d(tab, pts, cnt, shape, base.SRC, 2, base.STDDEV), pts, cnt


def measure_batch(im, lb, neg, neg_counts, bs, shape):
    tab, ctab = base._tables(im.device, bs, shape)
    hard = tab.clone()                                         # the last row: centred on a false positive of its slice
    hard[bs - 1, 11], hard[bs - 1, 12] = lits3d.FORCED_NEG, int(neg_counts[int(tab[bs - 1, 2])]) // 2
    status = torch.zeros(1, dtype=torch.int32, device=im.device)
    out = {"shape": dict(batch=bs, dhw=shape, crop=(int(shape[1] * base.ZOOM), int(shape[2] * base.ZOOM)), slices=base.SRC)}
    out["unflagged_batch_events"] = base._event_ms(lambda: base._batch(im, lb, tab, ctab, shape, status))
    out["flagged_batch_events"] = base._event_ms(lambda: _flagged(im, lb, neg, hard, ctab, shape, status))
    out["flagged_over_unflagged"] = out["flagged_batch_events"]["ms_median"] / out["unflagged_batch_events"]["ms_median"]
    images, labels, guide, pts, cnt = _flagged(im, lb, neg, hard, ctab, shape, status)
    assert int(status.item()) == 0
    negs_in_crop = 0
    for n in range(bs):                                        # every background click of a row with false positives is one
        row = hard[n].tolist()
        ch, cw = min(row[5], base.SRC[0]), min(row[6], base.SRC[1])
        z1 = min(max(row[2] - shape[0] // 2, 0), max(row[1] - shape[0], 0))
        y1, x1 = min(max(row[3] - ch // 2, 0), base.SRC[0] - ch), min(max(row[4] - cw // 2, 0), base.SRC[1] - cw)
        crop = neg[z1:z1 + shape[0], y1:y1 + ch, x1:x1 + cw]
        if int(crop.max()) > 0:
            negs_in_crop += 1
            for z, y, x in pts[n, 1, :int(cnt[n, 1])].tolist():
                assert int(crop[z, y, x]) > 0
    out["rows_with_false_positives"] = negs_in_crop
    kernels = base._by_kernel(lambda: _flagged(im, lb, neg, hard, ctab, shape, status))
    out["flagged_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    kernels = base._by_kernel(lambda: base._batch(im, lb, tab, ctab, shape, status))
    out["unflagged_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))

    argv = ("liver_3d --mode train --tag measure --model UNet3D --classes Liver Tumor --im_depth {} --im_height {} --im_width {} "
            "--im_channel 1 --batch_size {} --normalizer instance_norm --loss_weight_type numerical --loss_numeric_w 1 1 3 "
            "--use_spatial --local_enhance").format(shape[0], shape[1], shape[2], bs).split()
    args, _, _ = entry.get_arguments(argv)
    params = {"args": args}
    params.update(models.get_model_params(args, build_metrics=True))
    params.update(solver.get_solver_params(args))
    feats = {"images": images, "sp_guide": guide}
    out["unet3d_step_events"] = base._event_ms(lambda: models.model_fn(feats, labels, "train", params).loss)
    out["flagged_share_of_step"] = out["flagged_batch_events"]["ms_median"] / out["unet3d_step_events"]["ms_median"]
    print(shape, {k: v for k, v in out.items() if not k.endswith("kernels_ms")}, flush=True)
    print(shape, "flagged kernels", out["flagged_kernels_ms"], flush=True)
    print(shape, "unflagged kernels", out["unflagged_kernels_ms"], flush=True)
    return out


def measure_mining(lb):
    """unetk_fp_mask3d on 450 x 512 x 512: the labels are the store's case repeated along z; the prediction is the labelled
    tumour shifted by 3 columns plus 2500 false alarms, boxes of a random half-width 0 .. 4 per axis at random places."""
    reps = (MINE_DEPTH + base.DEPTH - 1) // base.DEPTH
    lab = lb.repeat(reps, 1, 1)[:MINE_DEPTH].contiguous()
    pred = torch.roll((lab >= 2 * lits.LB_SCALE).to(torch.uint8) * 2, 3, dims=2)
    rng = np.random.default_rng(3)
    for _ in range(2500):
        z, y, x = (int(rng.integers(0, n)) for n in lab.shape)
        hz, hy, hx = (int(v) for v in rng.integers(0, 5, 3))
        pred[max(z - hz, 0):z + hz + 1, max(y - hy, 0):y + hy + 1, max(x - hx, 0):x + hx + 1] = 2
    out = {"case": dict(dhw=tuple(lab.shape), predicted_voxels=int((pred >= 2).sum()), labelled_voxels=int((lab >= 128).sum()))}
    out["fp_mask3d_events"] = base._event_ms(lambda: ops.fp_mask3d(pred, lab, 2, 2, 6, lits.LB_SCALE, lits.LB_SCALE))
    a, b = ops.fp_mask3d(pred, lab, 2, 2, 6, lits.LB_SCALE, lits.LB_SCALE), ops.fp_mask3d(pred, lab, 2, 2, 6, lits.LB_SCALE, lits.LB_SCALE)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    out["head"] = a[2].tolist()
    assert int(a[1].sum()) == out["head"][2] == int((a[0] > 0).sum()) and out["head"][1] > 0
    kernels = base._by_kernel(lambda: ops.fp_mask3d(pred, lab, 2, 2, 6, lits.LB_SCALE, lits.LB_SCALE))
    out["kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    print("fp_mask3d", out, flush=True)
    return out


def main():
    dev = torch.device("cuda")
    im, lb = base._store(dev)
    neg, neg_counts = _neg_plane(lb)
    for bs, shape in base.SHAPES:
        OUT["x".join(str(v) for v in shape) + "_bs{}".format(bs)] = measure_batch(im, lb, neg, neg_counts, bs, shape)
        torch.cuda.empty_cache()
    OUT["fp_mask3d_450x512x512"] = measure_mining(lb)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no device: nothing to measure")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
