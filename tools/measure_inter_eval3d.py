"""Measure the 3-D interactive evaluator on one GPU: a synthetic 64 x 512 x 512 case, UNet3D at 10 x 256 x
256 x 1 with random weights, windows in batches of 4 (overlap 0.5: 12 x 3 x 3 = 108 windows, 27 tables), no mirrors.

    python tools/measure_inter_eval3d.py [--reps 10] [--max_iter 5]

Device events, medians of --reps: the click step (unetk_inter_click3d) in round 0 (no prediction), on a prediction whose
largest error region is a block with a hole at its mean (the fallback) and on the net's own prediction; the guide of one table
from 10 + 10 clicks (unetk_click_guide3d_list, K = 20); one round (click step, host read, 27 tables, finish).  Then the whole
session of the case through entry.main_eval_3d.run_session, in seconds.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.core import models  # noqa: E402
from boxsegliver_amd.data import lits  # noqa: E402
from boxsegliver_amd.entry import main_eval_3d  # noqa: E402

CASE = (64, 512, 512)
SHAPE = (10, 256, 256)


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def make_store(device):
    """One case: an object of two ellipsoids on a noisy image."""
    zz, yy, xx = np.ogrid[:CASE[0], :CASE[1], :CASE[2]]
    lab = (((zz - 26) / 18.) ** 2 + ((yy - 220) / 90.) ** 2 + ((xx - 230) / 70.) ** 2 <= 1) | \
          (((zz - 38) / 14.) ** 2 + ((yy - 290) / 50.) ** 2 + ((xx - 310) / 110.) ** 2 <= 1)
    lab = lab.astype(np.uint8)
    rng = np.random.default_rng(5)
    im = (rng.normal(240, 30, lab.shape) + 70 * lab).clip(1, 450) * lits.IM_SCALE
    return types.SimpleNamespace(im=torch.from_numpy(im.astype(np.uint16).view(np.int16)).to(device),
                                 lb=torch.from_numpy(lab * lits.LB_SCALE).to(device), device=device, offset={0: 0}), lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max_iter", type=int, default=5)
    opt = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    k = 20
    store, lab = make_store(device)
    out = {"case": list(CASE), "window": list(SHAPE), "batch": 4, "reps": opt.reps, "date": time.strftime("%Y-%m-%d")}
    args = main_eval_3d.get_arguments(("--mode eval --tag measure --model UNet3D --classes Liver --im_depth {} --im_height {} --im_width {} "
                                       "--im_channel 1 --batch_size 4 --normalizer instance_norm --use_spatial --local_enhance "
                                       "--stddev 1 3 3 --max_iter {}").format(SHAPE[0], SHAPE[1], SHAPE[2], k).split())
    mp = models.get_model_params(args)
    net = main_eval_3d.NetPredictor(mp["model"](args), mp.get("model_args", ()), mp.get("model_kwargs", {}), store, args)
    net.begin_case({"PID": 0, "size": list(CASE)})
    out["tables"], out["windows"] = len(net.tables), int(sum(len(t) for t in net.tables))
    pts = torch.full((2, k, 3), -1, dtype=torch.int32, device=device)
    cnt = torch.full((2,), 10, dtype=torch.int32, device=device)
    pts[:, :10, 0] = torch.randint(5, 60, (2, 10), dtype=torch.int32, device=device)
    pts[:, :10, 1:] = torch.randint(40, 470, (2, 10, 2), dtype=torch.int32, device=device)
    pred = net.binary(net.classes(pts, cnt))                            # builds the variables; the net's own prediction
    torch.cuda.synchronize()
    (dtab,) = lits.upload_pinned([net.tables[0]], device)
    out["guide_table_ms"] = median_ms(lambda: ops.click_guide3d_list(dtab, pts, cnt, SHAPE, CASE[1:], 2, (1., 3., 3.)), opt.reps)
    out["pass_ms"] = median_ms(lambda: net.classes(pts, cnt), 3)        # the 27 tables and the finish, guide included
    hollow = lab.copy()
    hollow[10:50, 100:400, 100:400] ^= 1                                # a 40 x 300 x 300 block of errors ...
    hollow[28:32, 246:254, 246:254] ^= 1                                # ... with a hole at its mean
    hollow = torch.from_numpy(hollow).to(device)
    ws = ops.inter_click3d_ws(ops.inter_click3d_desc(store.lb, 0, CASE[0], k, 1, lits.LB_SCALE), device)
    table = torch.empty(20, dtype=torch.int32, device=device)
    for name, p in (("click_round0_ms", None), ("click_fallback_ms", hollow), ("click_net_pred_ms", pred)):
        def step():
            cnt.zero_()
            return ops.inter_click3d(store.lb, 0, CASE[0], p, None, pts, cnt, 1, lits.LB_SCALE, table=table, ws=ws)
        out[name] = median_ms(step, opt.reps)
        row = step().cpu().numpy()
        out[name.replace("_ms", "_fallback")] = int(row[13])
        out[name.replace("_ms", "_components")] = int(row[3])

    def one_round():
        cnt.zero_()
        ops.inter_click3d(store.lb, 0, CASE[0], pred, None, pts, cnt, 1, lits.LB_SCALE, table=table, ws=ws)
        table.cpu()
        return net.classes(pts, cnt)
    out["round_ms"] = median_ms(one_round, 3)
    torch.cuda.synchronize()
    trace = []
    tic = time.perf_counter()
    inters, _ = main_eval_3d.run_session(store.lb, 0, CASE[0], lambda p, c: net.binary(net.classes(p, c)), opt.max_iter, 0.9, 1, trace, 0)
    torch.cuda.synchronize()
    out["case_s"] = time.perf_counter() - tic
    out["case_rounds"], out["case_inters"], out["case_max_iter"] = len(trace), inters, opt.max_iter
    out["case_fallbacks"] = int(sum(1 for r in trace if r[3]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
