"""The measurement of the geodesic click guide in DESIGN.md 7.3.7.1, taken in one process on one MI355X, on the store, the tables
and the clicks of tools/measure_lits_inter.py (LiTS-like content: noise over a body ellipse, a liver ellipse with tumour discs;
zoom 1.25 on 512 x 512 slices) at batch 16, 256 x 256 x 3:
  * `unetk_lits_inter_center` and `unetk_click_geodesic` alone, between device events, and their split by kernel;
  * the sweeps to convergence of the 2 x 16 solves of 100 batches with fresh tables and clicks: median and maximum;
  * one evaluation round at 512 x 512 (path 2: the fields in the workspace), 8 sessions with 10 clicks per kind;
  * one `liver_inter --use_spatial` UNetInter training step -- the batch kernels, forward, backward, Adam -- with the Euclidean
    guide and with --geodesic_guide, alternating in the same process.
Medians of 10.
Usage: python tools/measure_lits_geodesic.py [out.json]   (needs a GPU)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import measure_lits_inter as base  # noqa: E402
from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.core import models, solver  # noqa: E402
from boxsegliver_amd.data import lits, lits_inter  # noqa: E402
from boxsegliver_amd.entry import main as entry  # noqa: E402

OUT = {}
BS, SHAPE, SRC = 16, base.SHAPE, base.SRC
EVAL_BS, EVAL_HW, EVAL_CLICKS = 8, (512, 512), 10


def _tables(dev, seed):
    """One batch of BS samples as measure_lits_inter._tables lays it out, from `seed`; the click counts are drawn."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((BS, 16), np.int32)
    tab[:, 1] = base.DEPTH
    tab[:, 2] = rng.integers(1, base.DEPTH - 1, BS)
    tab[:, 3], tab[:, 4] = rng.integers(150, 360, BS), rng.integers(100, 330, BS)
    tab[:, 5], tab[:, 6] = int(SHAPE[1] * base.ZOOM), int(SHAPE[2] * base.ZOOM)
    tab[:, 7:9] = rng.integers(0, 2, (BS, 2))
    tab[:, 10] = rng.uniform(0.7, 1.5, BS).astype(np.float32).view(np.int32)
    tab[:BS // 2, 11], tab[:BS // 2, 12] = 1, rng.integers(0, 1000, BS // 2)
    clicks = lits_inter.draw_click_tab(rng, BS)
    return torch.from_numpy(tab).to(dev), torch.from_numpy(clicks.view(np.int32)).to(dev)


def _batch(im, lb, tab, ctab, status, geodesic):
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    images, labels = ops.lits_inter_batch(im, lb, tab, SHAPE, True, status, 2, 0.1, 7, lits.IM_SCALE, lits.LB_SCALE)
    pts, cnt = ops.lits_clicks(lb, tab, ctab, status, 2, lits_inter.CLICKS, lits.LB_SCALE)
    if geodesic:
        field = ops.lits_inter_center(im, tab, SHAPE, status, lits.IM_SCALE)
        guide = ops.click_geodesic(tab, field, pts, cnt, SHAPE[1:], 2, status=status, src_hw=SRC)
    else:
        guide = ops.click_guide(tab, pts, cnt, SHAPE[1:], SRC, 2, None)
    return images, labels, guide


def main():
    dev = torch.device("cuda")
    im, lb = base._store(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    tab, ctab = _tables(dev, 1)
    ops.lits_pick_voxels(lb, tab, 2, status, lits.LB_SCALE)
    pts, cnt = ops.lits_clicks(lb, tab, ctab, status, 2, lits_inter.CLICKS, lits.LB_SCALE)
    field = ops.lits_inter_center(im, tab, SHAPE, status, lits.IM_SCALE)
    OUT["shape"] = dict(batch=BS, hwc=SHAPE[1:] + SHAPE[:1], grid=tuple(field.shape[1:]), slices=SRC,
                        path=ops.click_geodesic_path(SHAPE[1:], SRC), clicks=cnt.cpu().numpy().tolist())

    # the two entries alone
    OUT["center_events"] = base._event_ms(lambda: ops.lits_inter_center(im, tab, SHAPE, status, lits.IM_SCALE))
    OUT["geodesic_events"] = base._event_ms(lambda: ops.click_geodesic(tab, field, pts, cnt, SHAPE[1:], 2, status=status, src_hw=SRC))
    OUT["euclidean_events"] = base._event_ms(lambda: ops.click_guide(tab, pts, cnt, SHAPE[1:], SRC, 2, None))
    kernels = base._by_kernel(lambda: (ops.lits_inter_center(im, tab, SHAPE, status, lits.IM_SCALE),
                                       ops.click_geodesic(tab, field, pts, cnt, SHAPE[1:], 2, status=status, src_hw=SRC)))
    OUT["kernels_ms"] = dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    print("alone", {k: OUT[k]["ms_median"] for k in ("center_events", "geodesic_events", "euclidean_events")}, flush=True)
    print("kernels", OUT["kernels_ms"], flush=True)

    # sweeps to convergence over 100 batches
    sweeps = []
    for seed in range(100, 200):
        t, c = _tables(dev, seed)
        ops.lits_pick_voxels(lb, t, 2, status, lits.LB_SCALE)
        p, n = ops.lits_clicks(lb, t, c, status, 2, lits_inter.CLICKS, lits.LB_SCALE)
        f = ops.lits_inter_center(im, t, SHAPE, status, lits.IM_SCALE)
        _, s = ops.click_geodesic(t, f, p, n, SHAPE[1:], 2, status=status, src_hw=SRC, want_sweeps=True)
        s = s.cpu().numpy()
        sweeps.extend(int(v) for v in s[n.cpu().numpy() > 0])
    OUT["sweeps"] = dict(solves=len(sweeps), median=statistics.median(sweeps), max=max(sweeps), min=min(sweeps),
                         bound=int(field.shape[1] * field.shape[2]))
    print("sweeps", OUT["sweeps"], flush=True)

    # one evaluation round at 512 x 512: whole slices, path 2
    etab = np.zeros((EVAL_BS, 16), np.int32)
    etab[:, 1], etab[:, 2] = base.DEPTH, np.arange(1, EVAL_BS + 1)
    etab[:, 3], etab[:, 4], etab[:, 5], etab[:, 6] = SRC[0] // 2, SRC[1] // 2, SRC[0], SRC[1]
    etab[:, 10] = np.array([1.0], np.float32).view(np.int32)[0]
    etab = torch.from_numpy(etab).to(dev)
    rng = np.random.default_rng(2)
    epts = np.full((EVAL_BS, 2, 20, 2), -1, np.int32)
    epts[:, :, :EVAL_CLICKS, 0] = rng.integers(100, 420, (EVAL_BS, 2, EVAL_CLICKS))
    epts[:, :, :EVAL_CLICKS, 1] = rng.integers(60, 440, (EVAL_BS, 2, EVAL_CLICKS))
    epts = torch.from_numpy(epts).to(dev)
    ecnt = torch.full((EVAL_BS, 2), EVAL_CLICKS, dtype=torch.int32, device=dev)
    eshape = (3,) + EVAL_HW
    efield = ops.lits_inter_center(im, etab, eshape, status, lits.IM_SCALE)
    _, es = ops.click_geodesic(etab, efield, epts, ecnt, EVAL_HW, 2, status=status, src_hw=SRC, want_sweeps=True)
    OUT["eval_round"] = dict(sessions=EVAL_BS, hw=EVAL_HW, grid=tuple(efield.shape[1:]), clicks_per_kind=EVAL_CLICKS,
                             path=ops.click_geodesic_path(EVAL_HW, SRC), sweeps_max=int(es.max()),
                             center_events=base._event_ms(lambda: ops.lits_inter_center(im, etab, eshape, status, lits.IM_SCALE)),
                             geodesic_events=base._event_ms(lambda: ops.click_geodesic(etab, efield, epts, ecnt, EVAL_HW, 2,
                                                                                       status=status, src_hw=SRC)))
    print("eval round", OUT["eval_round"], flush=True)

    # the training step, the batch kernels included, with either guide
    argv = ("liver_inter --mode train --tag measure --model UNetInter --classes Tumor --im_height {} --im_width {} --im_channel {} "
            "--batch_size {} --normalizer instance_norm --loss_weight_type numerical --loss_numeric_w 1 1 --use_spatial"
            ).format(SHAPE[1], SHAPE[2], SHAPE[0], BS).split()
    args, _, _ = entry.get_arguments(argv, guided=True)
    params = {"args": args}
    params.update(models.get_model_params(args, build_metrics=True))
    params.update(solver.get_solver_params(args))

    def step(geodesic):
        images, labels, guide = _batch(im, lb, tab, ctab, status, geodesic)
        return models.model_fn({"images": images, "sp_guide": guide}, labels, "train", params).loss

    runs = {False: [], True: []}
    for _ in range(3):                                                       # A B A B A B: drift shows as a trend within a key
        for geodesic in (False, True):
            runs[geodesic].append(base._event_ms(lambda: step(geodesic))["ms_median"])
    OUT["step_ms_euclidean"], OUT["step_ms_geodesic"] = runs[False], runs[True]
    extra = statistics.median(runs[True]) - statistics.median(runs[False])
    alone = OUT["center_events"]["ms_median"] + OUT["geodesic_events"]["ms_median"] - OUT["euclidean_events"]["ms_median"]
    OUT["step_extra_ms"], OUT["kernels_alone_extra_ms"] = extra, alone
    OUT["step_extra_allowed_ms"] = alone + 0.02 * statistics.median(runs[False])
    print("step", runs, "extra", extra, "the kernels alone", alone, "allowed", OUT["step_extra_allowed_ms"], flush=True)
    assert int(status.item()) == 0


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no device: nothing to measure")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
