"""Measure one round of the interactive evaluator on one GPU: batch 8, 512 x 512 slices, UNetInter at
256 x 256 x 3 with random weights, mirrors off and on.

    python tools/measure_inter_eval.py [--batch 8] [--slices 32] [--reps 10]

Device events, medians of --reps: the click step (unetk_inter_click) on the net's own predictions, on predictions whose
largest error region is a ring (every session takes the fallback) and on an empty error mask; the guide from 10 + 10 clicks
(unetk_click_guide_list, K = 20); the forward of the same batch, plain and under --eval_mirror --random_flip 3.  Then a whole
case of --slices object slices through entry.main_eval.run_case, in seconds.  Prints one JSON line."""
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
from boxsegliver_amd.entry import main_eval  # noqa: E402

SRC = 512


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


def make_store(n, device):
    """n slices: an object of two ellipses that drifts with z, on a noisy image."""
    yy, xx = np.ogrid[:SRC, :SRC]
    lab = np.zeros((n, SRC, SRC), np.uint8)
    for z in range(n):
        cy, cx = 200 + 3 * z, 230 - 2 * z
        lab[z] = (((yy - cy) / 90.) ** 2 + ((xx - cx) / 70.) ** 2 <= 1) | (((yy - cy - 60) / 50.) ** 2 + ((xx - cx - 80) / 110.) ** 2 <= 1)
    rng = np.random.default_rng(5)
    im = (rng.normal(240, 30, lab.shape) + 70 * lab).clip(1, 450) * lits.IM_SCALE
    return types.SimpleNamespace(im=torch.from_numpy(im.astype(np.uint16).view(np.int16)).to(device),
                                 lb=torch.from_numpy(lab * lits.LB_SCALE).to(device), device=device, offset={0: 0})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    opt = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    b, k = opt.batch, 20
    store = make_store(opt.slices, device)
    out = {"batch": b, "slice": [SRC, SRC], "net": [256, 256, 3], "reps": opt.reps, "date": time.strftime("%Y-%m-%d")}
    nets = {}
    for name, extra in (("plain", []), ("mirror", ["--eval_mirror"])):
        args = main_eval.get_arguments(("--mode eval --tag measure --model UNetInter --classes Liver --im_height 256 --im_width 256 "
                                        "--im_channel 3 --random_flip 3 --batch_size {} --normalizer instance_norm --use_spatial "
                                        "--local_enhance --stddev 5. --max_iter {}").format(b, k).split() + extra)
        mp = models.get_model_params(args)
        net = main_eval.NetPredictor(mp["model"](args), mp.get("model_args", ()), mp.get("model_kwargs", {}), store, args, 1)
        net.case = (0, opt.slices)
        nets[name] = net
    slot_slices = list(range(b))
    pts = torch.full((b, 2, k, 2), -1, dtype=torch.int32, device=device)
    cnt = torch.full((b, 2), 10, dtype=torch.int32, device=device)
    pts[:, :, :10] = torch.randint(40, 470, (b, 2, 10, 2), dtype=torch.int32, device=device)
    net = nets["plain"]
    pred = net(pts, cnt, slot_slices, slot_slices)                     # builds the images and the variables
    feats = {"images": net.images, "sp_guide": ops.click_guide_list(net.tab, pts, cnt, (256, 256), (SRC, SRC), 2, 5.0)}
    nets["mirror"].model = net.model                                   # the same variables under the mirrors
    out["forward_ms"] = median_ms(lambda: net.forward(feats), opt.reps)
    out["forward_mirror_ms"] = median_ms(lambda: nets["mirror"].probability(feats), opt.reps)
    out["guide_ms"] = median_ms(lambda: ops.click_guide_list(net.tab, pts, cnt, (256, 256), (SRC, SRC), 2, 5.0), opt.reps)
    rows = torch.tensor([[s, 1, -1, -1] for s in slot_slices], dtype=torch.int32, device=device)
    vol = torch.zeros((opt.slices, SRC, SRC), dtype=torch.uint8, device=device)
    lab256 = (store.lb[:b, ::2, ::2] > 0).to(torch.uint8).contiguous()
    ring = lab256.clone()
    ring[:, 96:160, 96:160] ^= 1                                        # a 128 x 128 block of errors ...
    ring[:, 126:130, 126:130] ^= 1                                      # ... with a hole at its mean
    ws = ops.inter_click_ws(ops.inter_click_desc(store.lb, b, (256, 256), k, 1, lits.LB_SCALE, 0, opt.slices), device)
    for name, p in (("click_net_pred_ms", pred), ("click_fallback_ms", ring), ("click_empty_ms", lab256), ("click_round0_ms", None)):
        def step():
            cnt.zero_()
            return ops.inter_click(store.lb, rows, p, pts, cnt, 1, lits.LB_SCALE, vol, 0, pred_hw=(256, 256), ws=ws)
        out[name] = median_ms(step, opt.reps)
        tab = step().cpu().numpy()
        out[name.replace("_ms", "_fallbacks")] = int(tab[:, 11].sum())
    for name in ("plain", "mirror"):
        p = nets[name]
        p.tab = None
        vol.zero_()
        torch.cuda.synchronize()
        trace = []
        tic = time.perf_counter()
        inters = main_eval.run_case(store.lb, list(range(opt.slices)), p, (256, 256), b, k, 0.9, 1, vol, 0, trace, 0)
        torch.cuda.synchronize()
        out["case_{}_s".format(name)] = time.perf_counter() - tic
        out["case_{}_session_rounds".format(name)] = len(trace)
        out["case_{}_inters".format(name)] = inters
    print(json.dumps(out))


if __name__ == "__main__":
    main()
