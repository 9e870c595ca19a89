"""Helpers of the slice-prior tests (test_slice_prior_host.py, test_gpu_slice_prior.py): the numpy / scipy restatement of what
`unetk_slice_prior_field` and `unetk_slice_prior_render` compute.

The reference's prior without --use_2d is plain numpy / scipy / skimage code.  skimage is not installed here, scipy is; each
step cites the reference lines it restates:
  boundary   skimage.segmentation.find_boundaries(prior, mode="inner") (DataLoader/NF/input_pipeline_3d.py:524,
             entry/main_eval_3d.py:355): dilation != erosion under the cross footprint, ANDed with the foreground -- restated
             with scipy.ndimage.grey_dilation / grey_erosion, whose default border rule (reflect) repeats the border pixel:
             like skimage's own padding, the border of the array never counts as background
  distance   input_pipeline_3d.py:525-527 (main_eval_3d.py:356-359), literally: scipy.ndimage.distance_transform_edt of the
             3-D array in which only slice z0 holds the boundary
  prior      :528 exp(-dist / 25) in float64; :530-532 --cascade_binary: the mask on slice z0, zeros elsewhere; :506-507 no
             foreground click: zeros
  resize     :443 resize_bilinear(align_corners) with the image, and the flips of :445-446 -- lits3d_ref's
The one rule that is the project's own: a slice without a boundary pixel (no object, or an object that fills the box) gives a
zero prior, where scipy's transform of an array without a seed returns an artefact (include/unetk.h)."""
import numpy as np
from scipy.ndimage import distance_transform_edt, generate_binary_structure, grey_dilation, grey_erosion

import lits3d_ref

SENTINEL = -1
CROSS = generate_binary_structure(2, 1)


def inner_boundary(mask):
    """find_boundaries(mask, mode="inner") for a 2-D 0 / 1 mask."""
    m = np.asarray(mask).astype(np.uint8)
    return (grey_dilation(m, footprint=CROSS) != grey_erosion(m, footprint=CROSS)) & (m != 0)


def boundary_brute(mask):
    """The rule as include/unetk.h states it, pixel by pixel: a foreground pixel with a background 4-neighbour inside the box."""
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    out = np.zeros_like(m)
    for y in range(h):
        for x in range(w):
            nb = [(y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)]
            out[y, x] = m[y, x] and any(0 <= i < h and 0 <= j < w and not m[i, j] for i, j in nb)
    return out


def d2_brute(boundary):
    """The exact squared 2-D distance to the nearest boundary pixel, int64 [h, w], by brute force over the boundary pixels."""
    by, bx = np.nonzero(boundary)
    h, w = boundary.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((yy[..., None] - by) ** 2 + (xx[..., None] - bx) ** 2).min(axis=-1)


def edt3d(boundary, z0, depth):
    """gen_kernel :525-527: the 3-D transform with only slice z0 seeded, float64 [depth, h, w]."""
    seeded = np.zeros((int(depth),) + boundary.shape, bool)
    seeded[z0] = boundary
    return distance_transform_edt(np.bitwise_not(seeded))


def field(mask, mode="boundary"):
    """What unetk_slice_prior_field writes for the box's mask (all zeros: no click / no such slice), int32 [h, w]: the squared
    distance of the reference's own transform on slice z0, rounded to the integer it is; SENTINEL without a boundary."""
    mask = np.asarray(mask)
    if mode == "binary":
        return (mask != 0).astype(np.int32)
    b = inner_boundary(mask)
    if not b.any():
        return np.full(mask.shape, SENTINEL, np.int32)
    return np.rint(edt3d(b, 0, 1)[0] ** 2).astype(np.int32)


def prior_volume(mask, z0, depth, mode="boundary"):
    """The prior at the box's resolution, float64 [depth, h, w] (:521-532): mask = the object on slice z0 of the box, all zeros
    without a foreground click."""
    mask = np.asarray(mask)
    out = np.zeros((int(depth),) + mask.shape, np.float64)
    if not 0 <= z0 < depth:
        return out
    if mode == "binary":
        out[z0] = mask != 0
        return out
    b = inner_boundary(mask)
    if not b.any():
        return out
    return np.exp(-edt3d(b, z0, depth) / 25)


def box_mask(lab, box, z0, obj_label, depth_out):
    """The object on crop slice z0 of the box (z1, y1, x1, ch, cw) of a case's labels uint8 [depth, src_h, src_w]; all
    background where z0 is no slice of the D-deep crop or lies at or beyond the case's depth."""
    z1, y1, x1, ch, cw = box
    if not 0 <= z0 < depth_out or z1 + z0 >= lab.shape[0]:
        return np.zeros((ch, cw), np.uint8)
    return (lab[z1 + z0, y1:y1 + ch, x1:x1 + cw] >= obj_label).astype(np.uint8)


def render(vol, out_hw, flips=(0, 0, 0)):
    """Channel 1 of unetk_slice_prior_render from the prior at crop resolution: the resize and the flips of the image."""
    return np.ascontiguousarray(lits3d_ref.flip(lits3d_ref.resize_bilinear(vol, out_hw), flips))
