"""Numpy restatement of the z-resampling kernels (include/unetk.h) for test_lits3d_zspace_host.py and
test_gpu_lits3d_zspace.py: `unetk_lits_patch3d_z` and its way back, `unetk_eval3d_accumulate_z` / `_wz`.  The in-plane steps
are those of lits3d_ref.py / eval3d_ref.py / eval3d_weighted_ref.py, imported; what is restated here is the z axis:

  crop box      z1 = min(max(cz - cd // 2, 0), max(depth - cd, 0)) with cd = min(max(zcrop, 1), zcrop_max); crop slices at or
                beyond the case's depth are zeros with label 0; the mask statistics run over the cd x ch x cw crop
  coordinates   float32, operation by operation: zs = float32((cd - 1) / (D - 1)) (0 for D == 1), in_z = float32(z) * zs,
                i0 = floor(in_z), i1 = min(i0 + 1, cd - 1), fz = in_z - float32(i0) -- lits3d_ref._coords, as y and x
  image         float64: v = v0 + fz (v1 - v0) of the two slices' in-plane values
  label         slice min(floor(in_z + 0.5), cd - 1) (roundf of a non-negative float32), in-plane nearest pixel
"""
import numpy as np

import eval3d_weighted_ref as wref
import lits3d_ref as ref


def clamp_cd(zcrop, zcrop_max):
    return min(max(int(zcrop), 1), int(zcrop_max))


def crop_box(center, crop_hw, cd, depth, src_hw):
    """(z1, y1, x1, ch, cw) of a cd-deep crop: lits3d_ref.crop_box with cd in place of D."""
    return ref.crop_box(center, crop_hw, (int(cd),), depth, src_hw)


def z_taps(n_in, n_out):
    """(i0, i1, f float64, nearest) of the n_out output coordinates on an axis of n_in: float32 coordinates."""
    c = ref._coords(n_in, n_out)
    i0 = np.floor(c).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    f = (c - i0.astype(np.float32)).astype(np.float64)
    near = np.minimum(np.floor(c.astype(np.float64) + 0.5).astype(np.int64), n_in - 1)
    return i0, i1, f, near


def patch(im, lab, center, crop_hw, shape, zcrop, zcrop_max=1 << 20, flips=(0, 0, 0), gamma=None, lab_max=2):
    """One sample of unetk_lits_patch3d_z: (image float64 [D, H, W], label int64 [D, H, W], m, s)."""
    d = int(shape[0])
    cd = clamp_cd(zcrop, zcrop_max)
    box = crop_box(center, crop_hw, cd, im.shape[0], im.shape[1:])
    img, lb = ref.crop(im, lab, box, cd)                            # [cd, ch, cw]; slices beyond the case are zeros
    z, m, s = ref.zscore(img)
    planes = ref.resize_bilinear(z, shape[1:])                      # [cd, H, W]: every crop slice's in-plane value
    lplanes = ref.resize_nearest(lb, shape[1:])
    i0, i1, f, near = z_taps(cd, d)
    out = planes[i0] + f[:, None, None] * (planes[i1] - planes[i0])
    out = ref.flip(out, flips)
    lb = np.minimum(ref.flip(lplanes[near], flips), lab_max)
    if gamma is not None:
        out = ref.augment_gamma(out, float(gamma))
    return np.ascontiguousarray(out), np.ascontiguousarray(lb), m, s


# ------------------------------------------------------------------------------------------------- the way back
def union_box(tab, zcrops, depth, src_hw):
    boxes = np.array([crop_box(r[2:5], r[5:7], cd, depth, src_hw) for r, cd in zip(tab, zcrops)])
    z1, y1, x1, ch, cw = boxes.T
    return (int(z1.min()), int(min((z1 + np.asarray(zcrops)).max(), depth)), int(y1.min()), int((y1 + ch).max()), int(x1.min()),
            int((x1 + cw).max()))


def resize_back(window, cd, crop_hw):
    """[D, H, W] -> [cd, ch, cw]: in-plane lits3d_ref.resize_bilinear per window slice, then the lerp along z."""
    planes = ref.resize_bilinear(window, crop_hw)                   # [D, ch, cw]
    i0, i1, f, _ = z_taps(window.shape[0], cd)
    return planes[i0] + f[:, None, None] * (planes[i1] - planes[i0])


class Sums(object):
    """acc float64 [depth, src_h, src_w, C]; wsum float64, hits int64, wmax float64 [depth, src_h, src_w] (wmax: the largest
    upper weight of a voxel's hits, as eval3d_weighted_ref.Sums)."""

    def __init__(self, depth, src_hw, c):
        vol = (int(depth),) + tuple(src_hw)
        self.acc, self.wsum = np.zeros(vol + (c,), np.float64), np.zeros(vol, np.float64)
        self.hits, self.wmax = np.zeros(vol, np.int64), np.zeros(vol, np.float64)


def accumulate(tab, zcrops, probs, shape, depth, src_hw, tables=None, sums=None):
    """tab int32 [N, 16], zcrops [N] (already clamped), probs [N, D, H, W, C] -> Sums, rows in order.  tables None: the
    unweighted entry (weights 1: wsum == hits); else (gz [D], gy [H], gx [W]) and the weight of a hit is
    lerp_z(gz) * lerp_y(gy) * lerp_x(gx) at the taps and fractions of the probabilities."""
    probs = np.asarray(probs, dtype=np.float64)
    c = probs.shape[-1]
    d = int(shape[0])
    s = Sums(depth, src_hw, c) if sums is None else sums
    for n, row in enumerate(np.asarray(tab)):
        cd = int(zcrops[n])
        z1, y1, x1, ch, cw = crop_box(row[2:5], row[5:7], cd, depth, src_hw)
        nz = max(min(cd, depth - z1), 0)                             # window slices below the case contribute nothing
        flips = tuple(int(v) for v in row[7:10])
        if tables is None:
            w = upper = np.ones((cd, ch, cw))
        else:
            gz = np.asarray(tables[0], dtype=np.float32).astype(np.float64)
            i0, i1, f, _ = z_taps(d, cd)
            wz, uz = gz[i0] + f * (gz[i1] - gz[i0]), np.where(f > 0, np.maximum(gz[i0], gz[i1]), gz[i0])
            (wy, uy), (wx, ux) = wref._axis_weights(tables[1], ch), wref._axis_weights(tables[2], cw)
            w = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
            upper = uz[:, None, None] * uy[None, :, None] * ux[None, None, :]
        place = (slice(z1, z1 + nz), slice(y1, y1 + ch), slice(x1, x1 + cw))
        for k in range(c):
            window = np.ascontiguousarray(ref.flip(probs[n, ..., k], flips))
            s.acc[place + (k,)] += (w * resize_back(window, cd, (ch, cw)))[:nz]
        s.wsum[place] += w[:nz]
        s.hits[place] += 1
        s.wmax[place] = np.maximum(s.wmax[place], upper[:nz])
    return s


K_LERP = 8.0     # one more nested fp32 lerp and its fraction: the step from 16 to 24 of the image bound (test_gpu_lits3d_zspace.py)


def bound(s, max_prob, weighted):
    """|acc - ref| per voxel and class, first order in u = 2^-24.  The hit is one more nested lerp than the bilerp of the plain
    entries, which eval3d_ref.bound carries as 16 u M (three nested lerps); the fourth lerp and its fraction add K_LERP u M,
    the same step the image bound of the patch takes from 16 to 24.
      unweighted: 2^-24 hits ((16 + 8) M + |ref|)                        (eval3d_ref.bound with 16 -> 24)
      weighted:   2^-24 hits ((K_ACC + 8 + 3) wmax M + |ref|)           (eval3d_weighted_ref.bound: 25 -> 36; the weight has a
                  third lerp of its own, 3 u wmax as wy and wx in that derivation)"""
    if weighted:
        k = wref.K_ACC + K_LERP + 3.0
        return 2.0 ** -24 * s.hits[..., None] * (k * s.wmax[..., None] * float(max_prob) + np.abs(s.acc))
    return 2.0 ** -24 * s.hits[..., None] * ((16.0 + K_LERP) * float(max_prob) + np.abs(s.acc))


def bound_wsum(s):
    """|wsum - ref| <= 2^-24 hits ((K_WSUM + 3) wmax + |ref|): eval3d_weighted_ref.bound_wsum with the third lerp."""
    return 2.0 ** -24 * s.hits * ((wref.K_WSUM + 3.0) * s.wmax + np.abs(s.wsum))
