"""Float64 numpy restatement of `unetk_eval3d_accumulate` (csrc/lits3d.hip) for test_eval3d_host.py and
test_gpu_eval3d.py: per table row the crop box of lits3d_ref.crop_box, the window un-flipped with lits3d_ref.flip, every
class volume resized back [D, H, W] -> [D, ch, cw] with lits3d_ref.resize_bilinear (float32 source coordinates, float64
lerps), added into the case for the slices below its depth; the coverage count goes up by one per row."""
import numpy as np

import lits3d_ref as ref


class HostStore(object):
    """What data/lits3d.eval_tables reads of a data/lits.SliceStore: the slices' extent and the cases' first slices."""

    def __init__(self, cases=None):
        cases = ref.make_cases() if cases is None else cases
        self.im, self.lb, base = ref.stack_store(cases)
        self.offset = {pid: int(b) for pid, b in enumerate(base)}
        self.meta = [{"PID": pid, "size": [int(c[0].shape[0]), ref.H, ref.W]} for pid, c in enumerate(cases)]


def row_box(row, shape, depth, src_hw):
    return ref.crop_box(row[2:5], row[5:7], shape, depth, src_hw)


def union_box(tab, shape, depth, src_hw):
    """(z0, z1, y0, y1, x0, x1) over the rows, z clipped to the case."""
    boxes = np.array([row_box(r, shape, depth, src_hw) for r in tab])
    z1, y1, x1, ch, cw = boxes.T
    return (int(z1.min()), int(min((z1 + shape[0]).max(), depth)), int(y1.min()), int((y1 + ch).max()), int(x1.min()),
            int((x1 + cw).max()))


def accumulate(tab, probs, shape, depth, src_hw, acc=None, cnt=None):
    """tab int32 [N, 16], probs [N, D, H, W, C] -> (acc float64 [depth, src_h, src_w, C], cnt int64 [depth, src_h, src_w]),
    added to the given ones, rows in order."""
    probs = np.asarray(probs, dtype=np.float64)
    c = probs.shape[-1]
    acc = np.zeros((depth,) + tuple(src_hw) + (c,), np.float64) if acc is None else acc
    cnt = np.zeros((depth,) + tuple(src_hw), np.int64) if cnt is None else cnt
    for n, row in enumerate(np.asarray(tab)):
        z1, y1, x1, ch, cw = row_box(row, shape, depth, src_hw)
        nz = max(min(int(shape[0]), depth - z1), 0)                  # a case shallower than D: the rest of the window is padding
        flips = tuple(int(v) for v in row[7:10])
        for k in range(c):
            window = np.ascontiguousarray(ref.flip(probs[n, ..., k], flips))     # a flip is its own inverse
            back = ref.resize_bilinear(window, (ch, cw))
            acc[z1:z1 + nz, y1:y1 + ch, x1:x1 + cw, k] += back[:nz]
        cnt[z1:z1 + nz, y1:y1 + ch, x1:x1 + cw] += 1
    return acc, cnt


def bound(ref_acc, cnt, max_prob):
    """|acc - ref| per voxel and class: three nested fp32 lerps per contribution (the constant of the image bound in
    test_gpu_lits3d.py) and cnt roundings of the running fp32 sum -- 2^-24 cnt (16 max|probs| + |ref|)."""
    return 2.0 ** -24 * cnt[..., None] * (16.0 * float(max_prob) + np.abs(ref_acc))


def top_two_gap(acc):
    s = np.sort(acc, axis=-1)
    return s[..., -1] - s[..., -2]
