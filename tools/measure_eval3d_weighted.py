"""The measurements of the weighted sliding-window evaluation in DESIGN.md 7.3.4, taken in one process on one MI355X:
  1. `unetk_eval3d_accumulate_w` against `unetk_eval3d_accumulate` on one batch of four 10 x 256 x 256 windows, C = 3, zoom
     1.125 (288 x 288 crops, union box 10 x 432 x 512), and `unetk_eval3d_finish` against `unetk_head_predict` + `cnt.min()`
     on the 64 x 512 x 512 case they belong to: the library's per-dispatch events, medians of 10; the two end-of-case steps
     also between device events, since `cnt.min()` is not a kernel of the library;
  2. (host only) the window tables served for a synthetic 64 x 512 x 512 case with and without a box.
Usage: python tools/measure_eval3d_weighted.py [out.json]   (part 1 needs a GPU)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boxsegliver_amd import ops  # noqa: E402
from boxsegliver_amd.data import lits3d  # noqa: E402

OUT = {}
SHAPE, C, CASE = (10, 256, 256), 3, (64, 512, 512)
REPS = 10


class _Store(object):
    """What eval_tables reads of a SliceStore."""

    def __init__(self, case):
        self.im = np.zeros((0,) + tuple(case[1:]), np.uint16)
        self.offset = {0: 0}


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
    per = [sum(ms[i0:i1]) for _, _, i0, i1, _ in recs] or list(ms)          # a wrapper without a record: one dispatch per call
    return dict(kernel=names[0], ms_median=statistics.median(per), ms_min=min(per), ms_max=max(per), reps=len(per))


def _event_ms(fn):
    for _ in range(3):
        fn()
    per = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b))
    return dict(ms_median=statistics.median(per), ms_min=min(per), ms_max=max(per), reps=len(per))


def part1():
    dev = torch.device("cuda")
    slices = torch.zeros(CASE, dtype=torch.int16, device=dev)
    case = {"PID": 0, "size": list(CASE)}
    tab = next(lits3d.eval_tables(case, _Store(CASE), SHAPE, 0.5, [(0, 0, 0)], 4,
                                  box=(0, 10, 0, 432, 0, 512)))            # y starts 0, 144; x starts 0, 224
    assert len(tab) == 4
    box = lits3d.table_box(tab, SHAPE, CASE[0], CASE[1:])
    assert box == (0, 10, 0, 432, 0, 512), box
    dtab = torch.from_numpy(tab).to(dev)
    probs = torch.softmax(torch.randn((4,) + SHAPE + (C,), device=dev), dim=-1).contiguous()
    tables = tuple(torch.from_numpy(g).to(dev) for g in lits3d.window_weights(SHAPE, 0.125))
    acc = torch.zeros(CASE + (C,), dtype=torch.float32, device=dev)
    cnt = torch.zeros(CASE, dtype=torch.int32, device=dev)
    wsum = torch.zeros(CASE, dtype=torch.float32, device=dev)
    nvox = (box[1] - box[0]) * (box[3] - box[2]) * (box[5] - box[4])
    mb = (probs.numel() * 4 + nvox * 8 * (C + 1)) / 1e6
    plain = _kernel_ms(lambda: ops.eval3d_accumulate(probs, dtab, SHAPE, 0, CASE[0], box, acc, cnt, slices, host_tab=tab))
    weighted = _kernel_ms(lambda: ops.eval3d_accumulate_w(probs, dtab, SHAPE, 0, CASE[0], box, tables, acc, wsum, slices, host_tab=tab))
    OUT["accumulate"] = dict(plain=plain, weighted=weighted, ratio=weighted["ms_median"] / plain["ms_median"], mb=mb,
                             table_bytes=4 * sum(SHAPE), tbps_plain=mb / plain["ms_median"] / 1e3,
                             tbps_weighted=mb / weighted["ms_median"] / 1e3)
    print("accumulate", OUT["accumulate"], flush=True)

    # the end of a case: every voxel covered
    acc.copy_(torch.rand_like(acc))
    cnt.fill_(1)
    wsum.fill_(0.5)
    whole = (0, CASE[0], 0, CASE[1], 0, CASE[2])
    unc = torch.zeros(1, dtype=torch.int32, device=dev)
    fin = {}
    fin["finish_wsum_kernel"] = _kernel_ms(lambda: ops.eval3d_finish(acc, wsum, whole, unc))
    fin["finish_cnt_kernel"] = _kernel_ms(lambda: ops.eval3d_finish(acc, cnt, whole, unc))
    fin["head_predict_kernel"] = _kernel_ms(lambda: ops.head_predict(acc.view(-1, C), C, want_preds=False))
    fin["finish_wsum_events"] = _event_ms(lambda: ops.eval3d_finish(acc, wsum, whole, unc))
    fin["finish_cnt_events"] = _event_ms(lambda: ops.eval3d_finish(acc, cnt, whole, unc))
    fin["head_predict_and_min_events"] = _event_ms(lambda: (ops.head_predict(acc.view(-1, C), C, want_preds=False), cnt.min()))
    fin["ratio_events"] = fin["finish_wsum_events"]["ms_median"] / fin["head_predict_and_min_events"]["ms_median"]
    fin["mb"] = (acc.numel() * 4 + wsum.numel() * 5) / 1e6
    assert int(unc.item()) == 0
    a = ops.eval3d_finish(acc, wsum, whole, unc)
    b, _ = ops.head_predict(acc.view(-1, C), C, want_preds=False)
    assert torch.equal(a.view(-1), b)
    OUT["finish"] = fin
    print("finish", fin, flush=True)


def part2():
    case = {"PID": 0, "size": list(CASE)}
    store = _Store(CASE)
    box = (10, 50, 100, 400, 60, 330)                                      # a liver-sized box: 40 x 300 x 270
    rows = {}
    for name, b in (("whole", None), ("box", box)):
        rows[name] = sum(len(t) for t in lits3d.eval_tables(case, store, SHAPE, 0.5, [(0, 0, 0)], 4, box=b))
    OUT["box_plan"] = dict(case=CASE, window=SHAPE, crop=lits3d.eval_windows(CASE[1:], SHAPE), box=box, windows_whole=rows["whole"],
                           windows_box=rows["box"], share=rows["box"] / rows["whole"])
    print("box plan", OUT["box_plan"], flush=True)


if __name__ == "__main__":
    part2()
    if torch.cuda.is_available():
        part1()
    else:
        print("no device: the kernel timings (part 1) are skipped")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)
