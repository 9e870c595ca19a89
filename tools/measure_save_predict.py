"""The three measurements of --save_predict in DESIGN.md 7.1.3, taken in one process on one MI355X:
  1. `unetk_nii_compose` on a synthetic 450 x 512 x 512 case (300 x 320 x 352 box), from the library's per-dispatch events;
  2. end of post-processing -> host buffer ready: compose + one copy against the literal host path, alternating;
  3. wall time of EvaluateVolume.run on the small test fixture with -s, without it, and with the writer joined per case.
Usage: python tools/measure_save_predict.py [out.json]   (needs a GPU; the fixture comes from tests/)"""
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.data import nii_kits  # noqa: E402

OUT = {}


def ellipsoid(box, radii_frac, centre_frac=(0.5, 0.5, 0.5)):
    z, y, x = np.ogrid[:box[0], :box[1], :box[2]]
    c = [f * n for f, n in zip(centre_frac, box)]
    r = [f * n for f, n in zip(radii_frac, box)]
    return ((((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2) <= 1).astype(np.uint8)


def part12():
    case, box, origin = (450, 512, 512), (300, 320, 352), (80, 100, 90)
    liver_h = ellipsoid(box, (0.48, 0.45, 0.45))
    tumor_h = ellipsoid(box, (0.08, 0.1, 0.1), (0.4, 0.55, 0.45)) * liver_h
    liver, tumor = torch.from_numpy(liver_h).cuda(), torch.from_numpy(tumor_h).cuda()
    n = case[0] * case[1] * case[2]
    hdr = nii_kits.header_from_meta(case, (1.0, 0.7, 0.7))
    for name, special in (("identity", False), ("x_flip", True)):
        tb, flips = nii_kits.file_orientation(hdr, special)
        out = torch.empty(n, dtype=torch.int16, device="cuda")
        for _ in range(3):
            ops.nii_compose(liver, tumor, origin, case, tb, flips, out=out)
        torch.cuda.synchronize()
        recs = []
        ops.profile_begin(64)
        ops.profile_on(recs)
        for _ in range(20):
            ops.nii_compose(liver, tumor, origin, case, tb, flips, out=out)
        torch.cuda.synchronize()
        ms, names = ops.profile_read()
        ops.profile_on(None)
        per = [sum(ms[i0:i1]) for _, _, i0, i1, _ in recs]
        med = statistics.median(per)
        OUT["kernel_" + name] = dict(kernel=names[0], ms_median=med, ms_min=min(per), ms_max=max(per),
                                     gbps_written=n * 2 / med / 1e6, mb_written=n * 2 / 1e6, reps=len(per))
        print("kernel", name, OUT["kernel_" + name], flush=True)
    # transposed path, for the record (file axis 0 along z)
    aff = np.zeros((3, 4))
    aff[0, 2], aff[1, 1], aff[2, 0] = -0.7, -0.7, 1.0
    hdr_t = nii_kits.Nifti1Header((case[0], case[1], case[2]), np.int16, sform=aff)
    tb, flips = nii_kits.file_orientation(hdr_t)
    for _ in range(2):
        ops.nii_compose(liver, tumor, origin, case, tb, flips, out=out)
    torch.cuda.synchronize()
    recs = []
    ops.profile_begin(64)
    ops.profile_on(recs)
    for _ in range(10):
        ops.nii_compose(liver, tumor, origin, case, tb, flips, out=out)
    torch.cuda.synchronize()
    ms, names = ops.profile_read()
    ops.profile_on(None)
    per = [sum(ms[i0:i1]) for _, _, i0, i1, _ in recs]
    OUT["kernel_transposed"] = dict(kernel=names[0], trans_bk=list(tb), ms_median=statistics.median(per), ms_min=min(per),
                                    gbps_written=n * 2 / statistics.median(per) / 1e6)
    print("kernel transposed", OUT["kernel_transposed"], flush=True)

    # end of post-processing -> host buffer ready, both paths alternating
    tb, flips = nii_kits.file_orientation(hdr, False)
    pinned = torch.empty(n, dtype=torch.int16, pin_memory=True)
    pad_with = tuple((o, c - o - b) for o, b, c in zip(origin, box, case))
    dev_t, host_t, host_parts = [], [], []
    for rep in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flat = ops.nii_compose(liver, tumor, origin, case, tb, flips, out=out)
        pinned.copy_(flat, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        a = liver.cpu().numpy()
        b = tumor.cpu().numpy()
        t2 = time.perf_counter()
        host_flat = nii_kits.to_file_order(np.pad(a + b, pad_with, mode="constant", constant_values=0), hdr, False)
        t3 = time.perf_counter()
        if rep == 0:
            assert np.array_equal(pinned.numpy(), host_flat)
            continue                                            # warm-up of both
        dev_t.append(t1 - t0)
        host_t.append(t3 - t1)
        host_parts.append((t2 - t1, t3 - t2))
    OUT["to_host_buffer"] = dict(device_ms=[1e3 * t for t in dev_t], host_ms=[1e3 * t for t in host_t],
                                 device_ms_median=1e3 * statistics.median(dev_t), host_ms_median=1e3 * statistics.median(host_t),
                                 host_copy_ms_median=1e3 * statistics.median(p[0] for p in host_parts),
                                 host_numpy_ms_median=1e3 * statistics.median(p[1] for p in host_parts))
    print("to host buffer", OUT["to_host_buffer"], flush=True)
    # for scale: the writer thread's gzip of this case (host only)
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory() as d:
        nii_kits.save_flat(pinned.numpy(), hdr.shape, hdr, os.path.join(d, "p.nii.gz"))
        size = os.path.getsize(os.path.join(d, "p.nii.gz"))
    OUT["gzip_level1"] = dict(seconds=time.perf_counter() - t0, bytes=size)
    print("gzip", OUT["gzip_level1"], flush=True)


def part3():
    import test_gpu_unet as t
    from test_lits_eval_host import _write_dataset
    from boxsegliver_amd.NetworksV2.UNet import UNet
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    with tempfile.TemporaryDirectory() as d:
        root = Path(d)
        pids = tuple(range(10))
        _write_dataset(root, pids=pids, depth=9, size=96)
        (root / "k_folds.txt").write_text("Fold 0:0\nFold 1:1\nFold 2:" + " ".join(str(p) for p in pids[2:]) + "\n")
        args = t.make_args(batch_size=4, im_height=64, im_width=64, eval_mirror=False, random_flip=0, metrics_eval=["Dice", "VOE"],
                           use_global_dice=False, pred_type="pred", mode="eval", eval_num=-1, save_path=None, test_fold=2,
                           filter_size=0, eval_skip_num=0, eval_in_patches=False, model="UNet")
        params = {"args": args, "model": UNet, "model_kwargs": dict(t.YML, num_down_samples=3), "model_args": (),
                  "lits_root": root, "proj_root": root}
        times = {"save": [], "plain": [], "save_joined": []}
        n_cases = None
        for rep in range(4):
            for variant in ("plain", "save", "save_joined"):
                e = ev.get_evaluator("Volume", estimator=None, model_dir=str(root / "{}{}".format(variant, rep)), params=params,
                                     volumes_on="device")
                e.save_join_each_case = variant == "save_joined"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.run(lits.input_fn_eval, checkpoint_path=None, save=variant != "plain")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                n_cases = e.calls
                if rep:
                    times[variant].append(dt)
        med = {k: statistics.median(v) for k, v in times.items()}
        OUT["eval_wall"] = dict(cases=n_cases, seconds=times, median=med,
                                added_ms_per_case=1e3 * (med["save"] - med["plain"]) / n_cases,
                                added_ms_per_case_joined=1e3 * (med["save_joined"] - med["plain"]) / n_cases)
        print("eval wall", OUT["eval_wall"], flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "these are measurements of the GPU path: no device, no numbers"
    part12()
    part3()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
