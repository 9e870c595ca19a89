"""Float64 numpy restatement of `unetk_eval3d_accumulate_w` and `unetk_eval3d_finish` (csrc/lits3d.hip) for
test_eval3d_weighted_host.py and test_gpu_eval3d_weighted.py; eval3d_ref.py restates the unweighted kernel and stays as it is.

Per table row: the window's weight volume is the outer product of gz and of gy, gx resized from H, W to the row's ch x cw
crop with the SAME bilinear taps as the probabilities (lits3d_ref.resize_bilinear: float32 source coordinates, float64
lerps), indexed in the un-flipped window; the un-flipped, resized-back probabilities are multiplied by it and added to the
case, the weights themselves to wsum."""
import numpy as np

import eval3d_ref
import lits3d_ref as ref

K_ACC = 25.0    # see bound()
K_WSUM = 8.0


def _axis_weights(g, n_out):
    """One axis of a row: (the table resized to n_out with the probabilities' taps, the larger of each voxel's two taps)."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    i0 = np.floor(ref._coords(len(g), n_out)).astype(np.int64)
    i1 = np.minimum(i0 + 1, len(g) - 1)
    return ref.resize_bilinear(g[None, None, :], (1, n_out))[0, 0, :], np.maximum(g[i0], g[i1])


def row_weights(tables, crop_hw, upper=False):
    """float64 [D, ch, cw]: gz[z] * lerp(gy)[y] * lerp(gx)[x] of one row, from the float32 tables as they are.  upper: with
    the larger tap in place of each lerp -- what the roundings of the weight are relative to (bound())."""
    gz = np.asarray(tables[0], dtype=np.float32).astype(np.float64)
    wy, wx = _axis_weights(tables[1], crop_hw[0])[int(upper)], _axis_weights(tables[2], crop_hw[1])[int(upper)]
    return gz[:, None, None] * wy[None, :, None] * wx[None, None, :]


class Sums(object):
    """What accumulate() carries from call to call: acc float64 [depth, src_h, src_w, C]; wsum float64, hits int64 and
    wmax float64 [depth, src_h, src_w] -- wmax: the largest upper weight (row_weights(upper=True)) of a voxel's hits."""

    def __init__(self, depth, src_hw, c):
        vol = (int(depth),) + tuple(src_hw)
        self.acc, self.wsum = np.zeros(vol + (c,), np.float64), np.zeros(vol, np.float64)
        self.hits, self.wmax = np.zeros(vol, np.int64), np.zeros(vol, np.float64)


def accumulate(tab, probs, tables, shape, depth, src_hw, sums=None):
    """tab int32 [N, 16], probs [N, D, H, W, C], tables (gz [D], gy [H], gx [W]) -> Sums, added to the given ones, rows in
    order."""
    probs = np.asarray(probs, dtype=np.float64)
    c = probs.shape[-1]
    s = Sums(depth, src_hw, c) if sums is None else sums
    for n, row in enumerate(np.asarray(tab)):
        z1, y1, x1, ch, cw = eval3d_ref.row_box(row, shape, depth, src_hw)
        nz = max(min(int(shape[0]), depth - z1), 0)
        flips = tuple(int(v) for v in row[7:10])
        w = row_weights(tables, (ch, cw))
        place = (slice(z1, z1 + nz), slice(y1, y1 + ch), slice(x1, x1 + cw))
        for k in range(c):
            window = np.ascontiguousarray(ref.flip(probs[n, ..., k], flips))
            back = ref.resize_bilinear(window, (ch, cw))
            s.acc[place + (k,)] += (w * back)[:nz]
        s.wsum[place] += w[:nz]
        s.hits[place] += 1
        s.wmax[place] = np.maximum(s.wmax[place], row_weights(tables, (ch, cw), upper=True)[:nz])
    return s


def bound(s, max_prob):
    """|acc - ref| per voxel and class <= 2^-24 hits (K_ACC wmax max|probs| + |ref|), first order in u = 2^-24, counted
    from the kernel's fp32 operations on one hit.  wmax is per voxel: the largest, over the voxel's hits, of
    gz[z] max(gy taps) max(gx taps) (Sums.wmax; 1 at most for tables with maximum 1) -- every rounding of a weight is
    relative to a value between its taps, so a voxel that only the rims of windows reach is held to its own small
    weights, not to the weight of a window's centre.  M = max|probs|, probs >= 0:
      * wy = a + f (b - a): a subtraction, a product, a sum, each rounding a value <= max(a, b) -> 3 u max(a, b); wx
        likewise; w = gz wy wx: two products -> |w - w_exact| <= (3 + 3 + 2) u wmax = 8 u wmax            (K_WSUM)
      * p = lits_bilerp: three nested lerps, 16 u M -- the constant of eval3d_ref.bound -> w |p - p_exact| <= 16 u wmax M
      * the product w p: 1 u wmax M          -> per hit (8 + 16 + 1) u wmax M = K_ACC u wmax M
      * the running sum: one rounding per hit of a partial sum <= |ref| (all terms are >= 0) -> hits u |ref|.
    A fused multiply-add in place of a product and a sum only drops roundings."""
    return 2.0 ** -24 * s.hits[..., None] * (K_ACC * s.wmax[..., None] * float(max_prob) + np.abs(s.acc))


def bound_wsum(s):
    """|wsum - ref| <= 2^-24 hits (K_WSUM wmax + |ref|): the same form, the weight's own error and the running sum."""
    return 2.0 ** -24 * s.hits * (K_WSUM * s.wmax + np.abs(s.wsum))


def finish(acc, weight, box):
    """-> (pred uint8 [depth, src_h, src_w], uncovered): argmax (lowest index on ties) where weight > 0 inside box, else 0;
    uncovered = voxels of box = (z0, z1, y0, y1, x0, x1) whose weight is not > 0."""
    inside = np.zeros(weight.shape, bool)
    inside[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
    covered = np.asarray(weight) > 0
    pred = np.where(inside & covered, np.argmax(acc, axis=-1), 0).astype(np.uint8)
    return pred, int((inside & ~covered).sum())


def write_prediction(directory, pid, mask, spacing=(2.5, 0.8, 0.8)):
    """predict-<pid>.nii.gz as _CaseSaver writes it: header from the case's size and spacing, nii_kits.to_file_order with
    the volume's mirror rule, save_flat."""
    from boxsegliver_amd.data import nii_kits
    hdr = nii_kits.header_from_meta(list(mask.shape), list(spacing))
    special = 28 <= int(pid) < 48
    trans_bk, _ = nii_kits.file_orientation(hdr, special)
    shape = nii_kits.data_shape(hdr)
    path = directory / "predict-{}.nii.gz".format(pid)
    nii_kits.save_flat(nii_kits.to_file_order(mask, hdr, special), tuple(shape[a] for a in trans_bk), hdr, path)
    return path
