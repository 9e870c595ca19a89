"""The measurement of the slice prior in DESIGN.md 7.3.11, taken in one process on one MI355X: the device time, between device
events, of one guided `liver_3d` training batch at 10 x 256 x 256 batch 4 and at one 96^3 patch (the store, the tables and the
clicks of tools/measure_lits3d_clicks.py: zoom 1.25 on 512 x 512 slices)
  * without a prior (`unetk_lits_pick_voxel` + `unetk_lits_patch3d` + `unetk_lits3d_clicks` + `unetk_click_guide3d`),
  * with --slice_prior boundary and with --slice_prior binary (+ `unetk_slice_prior_field` + `unetk_slice_prior_render`),
the split by kernel of the boundary batch (is the field slower than the click simulation it follows, and which of its two
passes dominates), and the added time of one evaluation round on a 64 x 512 x 512 case: the whole-slice field, built once per
session, and the shared-field render of every window table of the case (windows of 10 x 256 x 256, batch 4, no overlap).
Medians of 10.
Usage: python tools/measure_slice_prior.py [out.json]   (needs a GPU)"""
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
EVAL_DEPTH, EVAL_SHAPE, EVAL_BS = 64, (10, 256, 256), 4


def _guided(im, lb, tab, ctab, shape, status):
    images, labels = base._plain(im, lb, tab, shape, status)
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, 2, lits3d.CLICKS, lits.LB_SCALE)
    return images, labels, ops.click_guide3d(tab, pts, cnt, shape, base.SRC, 2, base.STDDEV), pts, cnt


def _with_prior(im, lb, tab, ctab, shape, status, mode):
    images, labels, guide, pts, cnt = _guided(im, lb, tab, ctab, shape, status)
    field, z0 = ops.slice_prior_field(lb, tab, pts, cnt, shape, 2, mode, lab_scale=lits.LB_SCALE)
    return ops.slice_prior_render(tab, images, field, z0, shape, base.SRC, mode), labels, guide, field


def measure(im, lb, bs, shape):
    tab, ctab = base._tables(im.device, bs, shape)
    status = torch.zeros(1, dtype=torch.int32, device=im.device)
    out = {"shape": dict(batch=bs, dhw=shape, crop=(int(shape[1] * base.ZOOM), int(shape[2] * base.ZOOM)), slices=base.SRC)}
    out["guided"] = base._event_ms(lambda: _guided(im, lb, tab, ctab, shape, status))
    for mode in ("boundary", "binary"):
        out["guided_" + mode] = base._event_ms(lambda: _with_prior(im, lb, tab, ctab, shape, status, mode))
        out["extra_ms_" + mode] = out["guided_" + mode]["ms_median"] - out["guided"]["ms_median"]
    plain = _guided(im, lb, tab, ctab, shape, status)
    images, labels, guide, field = _with_prior(im, lb, tab, ctab, shape, status, "boundary")
    assert torch.equal(images[..., 0], plain[0][..., 0]) and torch.equal(labels, plain[1]) and torch.equal(guide, plain[2])
    assert int(status.item()) == 0 and float(images[..., 1].max()) > 0.9 and int(field.max()) > 0
    kernels = base._by_kernel(lambda: _with_prior(im, lb, tab, ctab, shape, status, "boundary"))
    out["boundary_kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    clicks = sum(v for k, v in kernels.items() if "clk3_" in k)
    prior = {k: v for k, v in kernels.items() if "sp_" in k}
    out["click_simulation_ms"], out["prior_kernels_ms"] = clicks, prior
    out["field_exceeds_click_simulation"] = sum(v for k, v in prior.items() if "render" not in k) > clicks
    print(shape, {k: v for k, v in out.items() if k != "boundary_kernels_ms"}, flush=True)
    print(shape, "kernels", out["boundary_kernels_ms"], flush=True)
    return out


def measure_eval(im, lb):
    """One evaluation round's added time on a case of 64 slices: the field once, and the render of every window table."""
    class _Store(object):
        offset = {0: 0}
    store = _Store()
    store.im, store.lb, store.device = im[:EVAL_DEPTH], lb[:EVAL_DEPTH], im.device
    case = {"PID": 0, "size": [EVAL_DEPTH, base.SRC[0], base.SRC[1]]}
    tables = [torch.from_numpy(t).to(im.device) for t in lits3d.eval_tables(case, store, EVAL_SHAPE, 0.0, [(0, 0, 0)], EVAL_BS)]
    pts = torch.full((2, 20, 3), -1, dtype=torch.int32, device=im.device)
    pts[0, 0] = torch.tensor([EVAL_DEPTH // 2, 230, 180], dtype=torch.int32)
    cnt = torch.tensor([1, 0], dtype=torch.int32, device=im.device)
    patches = [ops.lits_patch3d(store.im, store.lb, t, EVAL_SHAPE, False, 2, lits.IM_SCALE, lits.LB_SCALE)[0] for t in tables]
    out = {"case": dict(dhw=(EVAL_DEPTH,) + base.SRC, windows=EVAL_SHAPE, batch=EVAL_BS, tables=len(tables),
                        rows=int(sum(t.shape[0] for t in tables)))}
    for mode in ("boundary", "binary"):
        out["field_once_" + mode] = base._event_ms(
            lambda: ops.slice_prior_field(store.lb, tables[0][:1].contiguous(), pts, cnt, EVAL_SHAPE, 2, mode, whole=True))
        field, z0 = ops.slice_prior_field(store.lb, tables[0][:1].contiguous(), pts, cnt, EVAL_SHAPE, 2, mode, whole=True)
        out["render_all_tables_" + mode] = base._event_ms(
            lambda: [ops.slice_prior_render(t, p, field, z0, EVAL_SHAPE, base.SRC, mode, shared=True) for t, p in zip(tables, patches)])
    print("evaluation round", out, flush=True)
    return out


def main():
    dev = torch.device("cuda")
    im, lb = base._store(dev)
    for bs, shape in base.SHAPES:
        OUT["x".join(str(v) for v in shape) + "_bs{}".format(bs)] = measure(im, lb, bs, shape)
        torch.cuda.empty_cache()
    OUT["eval_round_64x512x512"] = measure_eval(im, lb)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no device: nothing to measure")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
