"""Time one LiTS-sized case (450x512x512, liver + tumor) through the volume evaluator's scoring, host against device:
_postprocess + ConfusionMatrix + metric_3d (all six metrics) per class against _score_case_device.
Needs a GPU.  Usage: python tools/measure_eval_device.py   (prints one JSON object)"""
import json
from collections import defaultdict
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import argparse  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boxsegliver_amd import loss_metrics, ops  # noqa: E402
from boxsegliver_amd.evaluators import evaluator_liver as ev  # noqa: E402


class _M(object):
    classes = ["Background", "Liver", "Tumor"]


def case():
    D, H, W = 450, 512, 512
    z, y, x = np.ogrid[:D, :H, :W]
    rng = np.random.default_rng(0)
    lab = np.zeros((D, H, W), np.uint8)
    lab[((z - 220) / 150.0) ** 2 + ((y - 250) / 120.0) ** 2 + ((x - 230) / 140.0) ** 2 <= 1.0] = 1
    lab[((z - 200) / 20.0) ** 2 + ((y - 240) / 25.0) ** 2 + ((x - 220) / 18.0) ** 2 <= 1.0] = 2
    pred = np.zeros((D, H, W), np.uint8)
    pred[((z - 224) / 148.0) ** 2 + ((y - 247) / 121.0) ** 2 + ((x - 233) / 139.0) ** 2 <= 1.0] = 1
    pred[((z - 203) / 21.0) ** 2 + ((y - 243) / 24.0) ** 2 + ((x - 222) / 19.0) ** 2 <= 1.0] = 2
    s = rng.integers(0, [D, H, W], size=(4000, 3))
    pred[s[:, 0], s[:, 1], s[:, 2]] = rng.integers(1, 3, 4000)
    return pred, lab


def main():
    args = argparse.Namespace(eval_mirror=False, random_flip=0, use_global_dice=False, pred_type="pred", mode="eval",
                              metrics_eval=["Dice", "VOE", "RVD", "ASSD", "RMSD", "MSD"])
    e = ev.EvaluateVolume(estimator=None, model_dir=".", params={"args": args, "model_instances": [_M()]})
    pred, lab = case()
    req = args.metrics_eval
    out = {}

    def device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e._score_case_device(pred, lab, False, defaultdict(int), False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    e.clear_metrics()
    device()                                              # warm-up (library load, allocator)
    times = []
    for _ in range(3):
        e.clear_metrics()
        times.append(device())
    dev_vals = {k: v[-1] for k, v in e.metric_values.items()}
    out["device_s"] = times
    # the device steps one by one
    p = torch.from_numpy(pred).cuda()
    l = torch.from_numpy(lab).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter(); v = e._postprocess_device(p); torch.cuda.synchronize(); out["dev_postprocess_s"] = time.perf_counter() - t0
    lb = e._postprocess_device(l, is_label=True)
    t0 = time.perf_counter(); ops.mask_counts(v["Liver"], lb["Liver"]); out["dev_counts_s"] = time.perf_counter() - t0
    t0 = time.perf_counter(); loss_metrics.metric_3d_device(v["Liver"], lb["Liver"], required=req); out["dev_metric3d_liver_s"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    hv = e._postprocess(pred)
    out["host_postprocess_s"] = time.perf_counter() - t0
    hl = e._postprocess(lab, is_label=True)
    host_vals = {}
    t0 = time.perf_counter()
    conf = loss_metrics.ConfusionMatrix(hv["Liver"].astype(int), hl["Liver"].astype(int)); conf.compute()
    out["host_confusion_s"] = time.perf_counter() - t0
    for cls in ("Liver", "Tumor"):
        t0 = time.perf_counter()
        for k, val in loss_metrics.metric_3d(hv[cls], hl[cls], required=req).items():
            host_vals["{}/{}".format(cls, k)] = val
        out["host_metric3d_{}_s".format(cls)] = time.perf_counter() - t0
    out["max_rel_diff"] = max(abs(dev_vals[k] - host_vals[k]) / max(abs(host_vals[k]), 1e-300) for k in host_vals)
    out["values"] = {k: float(v) for k, v in host_vals.items()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
