"""The measurements of `liver_3d --mode infer` in DESIGN.md 7.3.15, taken in one process on one MI355X, on a synthetic
450 x 512 x 512 int16 case written both uncompressed and as .nii.gz:
  1. `unetk_nii_ingest` on the t0 == 2 path (the LiTS orientation, x mirrored as for cases 28..47) and on one transposed
     orientation (file axis 0 along z): the library's per-dispatch events, medians of 10, and the achieved bytes / s (the block
     read once, the slices written once);
  2. the host route it replaces on the same machine -- nii_kits.read_nii + the store's encoding + one upload -- against the
     device route -- voxel block into pinned memory, upload, ingest -- for both files: wall time, medians of 5 (a host pass
     takes seconds);
  3. `unetk_eval3d_prob` on the case's accumulator (C = 3): per-dispatch events, medians of 10;
  4. wall time per case of the whole run (entry point, a four-step UNet3D, windows of 8 x 128 x 128 without overlap) over three
     copies of the .gz case, with and without the read-ahead thread (the run's start-up, the same in both, is shared out).
Usage: python tools/measure_infer3d.py [out.json]   (needs a GPU; the training fixture of part 4 comes from tests/)"""
import json
import os
import shutil
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
from boxsegliver_amd.data import lits3d, nii_kits  # noqa: E402

OUT = {}
CASE = (450, 512, 512)
REPS = 10
HOST_REPS = 5


def _kernel_ms(fn):
    """Median, min and max over REPS calls of the time of the library's dispatches in fn()."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    recs = []
    ops.profile_begin(8 * REPS)
    ops.profile_on(recs)
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    ms, names = ops.profile_read()
    ops.profile_on(None)
    per = [sum(ms[i0:i1]) for _, _, i0, i1, _ in recs] or list(ms)
    return dict(kernel=names[0], ms_median=statistics.median(per), ms_min=min(per), ms_max=max(per), reps=len(per))


def _wall(fn, reps):
    fn()                                                    # warm-up: page cache, pinned buffers, allocator
    per = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append(time.perf_counter() - t0)
    return dict(seconds=per, median=statistics.median(per))


def synthetic_case(directory):
    """A CT-like volume (smooth body, organ, noise of a few HU: it deflates about as a scan does) as volume-30.nii[.gz]."""
    rng = np.random.default_rng(0)
    d, h, w = CASE
    z, y, x = np.ogrid[:d, :h, :w]
    body = (((y - 256) / 230.0) ** 2 + ((x - 256) / 250.0) ** 2) <= 1
    organ = (((z - 225) / 150.0) ** 2 + ((y - 230) / 90.0) ** 2 + ((x - 180) / 110.0) ** 2) <= 1
    hu = np.where(body, 40, -1000).astype(np.int16) + organ.astype(np.int16) * 60
    hu += rng.integers(-12, 13, CASE, dtype=np.int16)
    header = nii_kits.header_from_meta(CASE, (1.0, 0.7, 0.7))
    flat = nii_kits.to_file_order(hu, header, True)
    paths = (Path(directory) / "volume-30.nii", Path(directory) / "volume-30.nii.gz")
    for p in paths:
        nii_kits.save_flat(flat, header.shape, header, p)
    OUT["case"] = dict(shape=list(CASE), nii_bytes=paths[0].stat().st_size, gz_bytes=paths[1].stat().st_size)
    print("case", OUT["case"], flush=True)
    return paths, hu


def part1(paths):
    plan = lits3d.infer_plan(paths[0])
    host = np.empty(plan["nbytes"], np.uint8)
    lits3d.read_voxel_block(paths[0], plan["header"], host)
    block = torch.from_numpy(host).cuda()
    out = torch.empty(CASE, dtype=torch.int16, device="cuda")
    moved = 2 * plan["nbytes"]
    r = _kernel_ms(lambda: ops.nii_ingest(block, plan["dtype"], plan["file_shape"], plan["trans_bk"], plan["flips"], out=out))
    r["gbps"] = moved / r["ms_median"] / 1e6
    OUT["ingest_rows"] = r
    print("ingest t0 == 2", r, flush=True)
    aff = np.zeros((3, 4))
    aff[0, 2], aff[1, 1], aff[2, 0] = -0.7, -0.7, 1.0                                       # file axis 0 runs along z
    hdr_t = nii_kits.Nifti1Header(CASE, np.int16, sform=aff)
    tb, flips = nii_kits.file_orientation(hdr_t)
    out_t = torch.empty(nii_kits.data_shape(hdr_t), dtype=torch.int16, device="cuda")
    r = _kernel_ms(lambda: ops.nii_ingest(block, np.dtype(np.int16), CASE, tb, flips, out=out_t))
    r.update(gbps=moved / r["ms_median"] / 1e6, trans_bk=list(tb))
    OUT["ingest_transposed"] = r
    print("ingest transposed", r, flush=True)
    return out


def part2(paths, hu, ingested):
    lo, hi, scale = ops.STORE_WINDOW
    keep = {}

    def host_route(path):
        _, data = nii_kits.read_lits(30, "vol", path)
        enc = ((np.clip(data, lo, hi) - lo) * scale).astype(np.uint16)
        keep["host"] = torch.from_numpy(enc.view(np.int16)).cuda()

    reader = {}

    def device_route(path):
        r = reader.setdefault(path, lits3d.VolumeReader([path], torch.device("cuda"), ahead=False))
        plan, block = r.get(0)
        dev = block.cuda(non_blocking=True)
        r.sent(0)
        keep["device"] = ops.nii_ingest(dev, plan["dtype"], plan["file_shape"], plan["trans_bk"], plan["flips"],
                                        plan["header"].scl_slope, plan["header"].scl_inter)
    for path in paths:
        kind = "gz" if str(path).endswith(".gz") else "nii"
        h = _wall(lambda: host_route(path), HOST_REPS)
        d = _wall(lambda: device_route(path), HOST_REPS)
        assert torch.equal(keep["host"], keep["device"]) and torch.equal(keep["device"], ingested)
        OUT["route_" + kind] = dict(host=h, device=d, speedup=h["median"] / d["median"])
        print("route", kind, OUT["route_" + kind], flush=True)
    for r in reader.values():
        r.close()


def part3():
    d, h, w = CASE
    acc = torch.rand((d, h, w, 3), device="cuda")
    cnt = torch.randint(1, 9, (d, h, w), dtype=torch.int32, device="cuda")
    acc *= cnt.unsqueeze(-1)
    out = torch.empty(d * h * w, dtype=torch.uint8, device="cuda")
    r = _kernel_ms(lambda: ops.eval3d_prob(acc, cnt, 1, None, (2, 1, 0), (True, False, False), out=out))
    r["gbps_algorithmic"] = (d * h * w * (4 + 4 + 1)) / r["ms_median"] / 1e6                 # one class, the weight, the bytes written
    OUT["eval3d_prob"] = r
    print("eval3d_prob", r, flush=True)


def part4(paths):
    import lits3d_ref as ref
    from boxsegliver_amd.entry import main as entry
    with tempfile.TemporaryDirectory() as d:
        root = Path(d)
        ref.write_dataset(root)
        argv = ("liver_3d --mode train --tag m --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
                "--im_width 32 --im_channel 1 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm --num_of_steps 4 "
                "--batches_per_epoch 2 --evaluator Volume --learning_rate 0.001 --log_step 1").split()
        argv += ["--lits_root", str(root), "--model_dir", str(root / "run")]
        assert entry.main(argv) == 0
        copies = []
        for k in (1, 2, 3):
            copies.append(root / "scan-{}.nii.gz".format(k))
            shutil.copyfile(paths[1], copies[-1])
        ev = list(argv)
        ev[ev.index("--mode") + 1] = "infer"
        for flag, value in (("--batch_size", "8"), ("--im_depth", "8"), ("--im_height", "128"), ("--im_width", "128")):
            ev[ev.index(flag) + 1] = value
        ev += ["--eval_final", "--save_predict", "--eval_overlap", "0", "--infer_volumes"] + [str(c) for c in copies]
        times = {True: [], False: []}
        for rep in range(3):
            for ahead in (True, False):
                args, sub, pipe = entry.get_arguments(ev + ["--save_path", "p{}{}".format(rep, int(ahead))])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                entry.run(args, sub, pipe, dataset_params={"infer_read_ahead": ahead})
                torch.cuda.synchronize()
                if rep:
                    times[ahead].append((time.perf_counter() - t0) / len(copies))
        OUT["wall_per_case"] = dict(cases=len(copies), window=[8, 128, 128], overlap=0.0, with_thread=times[True],
                                    without_thread=times[False], median_with=statistics.median(times[True]),
                                    median_without=statistics.median(times[False]))
        print("wall per case", OUT["wall_per_case"], flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "these are measurements of the GPU path: no device, no numbers"
    with tempfile.TemporaryDirectory() as tmp:
        files, volume = synthetic_case(tmp)
        resident = part1(files)
        part2(files, volume, resident)
        del resident
        part3()
        torch.cuda.empty_cache()
        part4(files)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
