"""The measurement of per-lesion detection in DESIGN.md 7.1.4, taken in one process on one MI355X: one synthetic
450 x 512 x 512 case with a few dozen lesions, scored by loss_metrics.tumor_detection_metrics_device (labelling both masks,
the overlap table, one table read, the matching on the host) and by loss_metrics.tumor_detection_metrics on the host for the
same masks.  Prints the workspace size, the device time between events (kernels only) and on the wall clock (with the
table read and the matching), the time of every dispatch of one call, and the host time; the two dicts must be equal.
Usage: python tools/measure_detection.py [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boxsegliver_amd import _abi, loss_metrics, ops  # noqa: E402

CASE = (450, 512, 512)
LESIONS, REPS = 40, 5
OUT = {}


def _ball(mask, centre, radius):
    lo = [max(0, int(c - radius)) for c in centre]
    hi = [min(s, int(c + radius) + 1) for c, s in zip(centre, mask.shape)]
    z, y, x = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= \
        (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius ** 2


def synthetic_case(seed=0):
    """(prediction, labels) uint8: LESIONS balls of radius 3..20 in the labels; the prediction finds three quarters of them a
    little displaced and resized, splits a few in two, and adds small false alarms."""
    rng = np.random.default_rng(seed)
    ref, res = np.zeros(CASE, bool), np.zeros(CASE, bool)
    for k in range(LESIONS):
        c = [int(rng.integers(40, s - 40)) for s in CASE]
        r = float(rng.uniform(3, 20))
        _ball(ref, c, r)
        if k % 4 != 3:
            _ball(res, [v + int(rng.integers(-2, 3)) for v in c], r * float(rng.uniform(0.7, 1.2)))
            if k % 8 == 0:
                res[:, c[1], :] = False                         # cut through the centre: two result objects on one lesion
    for _ in range(25):
        _ball(res, [int(rng.integers(10, s - 10)) for s in CASE], float(rng.uniform(1, 3)))
    return res.view(np.uint8), ref.view(np.uint8)


def main():
    res, ref = synthetic_case()
    dev = torch.device("cuda")
    r, f = torch.from_numpy(res).to(dev), torch.from_numpy(ref).to(dev)
    OUT["case"] = CASE
    OUT["ws_bytes"] = int(_abi.lib().unetk_component_overlaps_ws_bytes(*CASE, 65536, 262144))
    OUT["table_bytes"] = 4 * (4 + 4 * 65536 + 3 * 262144)
    for _ in range(2):
        got = loss_metrics.tumor_detection_metrics_device(r, f)
    torch.cuda.synchronize()
    ws = torch.empty(OUT["ws_bytes"], dtype=torch.uint8, device=dev)
    table = torch.empty(OUT["table_bytes"] // 4, dtype=torch.int32, device=dev)
    kernels, wall = [], []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ops.component_overlaps_table(r, f, table=table, ws=ws)
        b.record()
        torch.cuda.synchronize()
        kernels.append(a.elapsed_time(b))
        t0 = time.perf_counter()
        got = loss_metrics.tumor_detection_metrics_device(r, f)
        wall.append((time.perf_counter() - t0) * 1e3)
    OUT["device_kernels_ms"] = dict(median=statistics.median(kernels), min=min(kernels), max=max(kernels), reps=REPS)
    OUT["device_wall_ms"] = dict(median=statistics.median(wall), min=min(wall), max=max(wall), reps=REPS)
    recs = []
    ops.profile_begin(64)
    ops.profile_on(recs)
    ops.component_overlaps_table(r, f, table=table, ws=ws)
    torch.cuda.synchronize()
    ms, names = ops.profile_read()
    ops.profile_on(None)
    OUT["dispatches_ms"] = [[n.replace("(anonymous namespace)::", "").split("(")[0], round(m, 4)] for n, m in zip(names, ms)]
    head = table[:4].tolist()
    OUT["head"] = head
    t0 = time.perf_counter()
    want = loss_metrics.tumor_detection_metrics(res, ref)
    OUT["host_ms"] = (time.perf_counter() - t0) * 1e3
    OUT["device"], OUT["host"] = got, want
    assert got == want, (got, want)
    print("workspace {:.2f} GB, table {:.1f} MB; components res / ref / pairs = {} / {} / {}".format(
        OUT["ws_bytes"] / 1e9, OUT["table_bytes"] / 1e6, *head[:3]))
    print("device: kernels {:.2f} ms (median of {}), with the table read and the matching {:.2f} ms".format(
        OUT["device_kernels_ms"]["median"], REPS, OUT["device_wall_ms"]["median"]))
    for n, m in OUT["dispatches_ms"]:
        print("  {:<28s} {:8.4f} ms".format(n, m))
    print("host: {:.0f} ms; {}".format(OUT["host_ms"], want))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("tools/measure_detection.py needs a GPU")
    main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
