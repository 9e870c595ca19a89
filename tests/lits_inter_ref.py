"""Helpers of the click-guided LiTS pipeline tests (test_lits_inter_host.py, test_gpu_lits_inter.py): the float64 / integer
numpy restatement of what `unetk_lits_inter_batch`, `unetk_lits_clicks` and `unetk_click_guide` compute.

TensorFlow does not run here, so the restatement is builder-written ("parity unpinned"), except `crop_box` and
`clicks`: the reference's img_crop, gen_kernel and inter_simulation are plain numpy / scipy and do run in the build container,
and test_ref_clicks_host.py holds both to what they gave (tests/golden/ref_clicks.json).  Each step cites the reference lines
it restates:
  crop       DataLoader/misc.py:108-129 img_crop: slices cz - C/2 .. cz + C/2, zero padding outside the case (no shift); the
             (y, x) box clamped to the slice
  z-score    DataLoader/NF/input_pipeline_g_simply.py:437-442 (lits3d_ref.zscore; an empty mask gives zeros)
  resize     :466-469 resize_bilinear / :513-515 resize_nearest_neighbor, align_corners=True (lits3d_ref)
  flips      :498-499, utils/image_ops.py:287-314
  gamma      :518-519, utils/image_ops.py:339-354 augment_gamma(retain_stats=True) over the whole [H, W, C] image
  noise      :521-524, utils/image_ops.py:209-238 random_noise with the library's counter generator (unetk_rng), then the
             channel mask
  clicks     :346-412 inter_simulation as :530-561 gen_kernel calls it, np.random replaced by explicit draws, scipy's
             binary_erosion used literally
  guide      utils/image_ops.py:396-434 create_spatial_guide_2d, then the resize and the flips of the image
"""
import numpy as np
from scipy.ndimage import binary_erosion

import lits3d_ref
import unetk_rng
from lits3d_ref import (IM_SCALE, LB_SCALE, augment_gamma, make_cases, resize_bilinear, resize_nearest,  # noqa: F401
                        stack_store, table_row, write_dataset, zscore)

MAX_CLICKS = 4
CLICK_TAB_COLS = 12


# ------------------------------------------------------------------------------------------------- crop
def crop_box(center_yx, crop_hw, src_hw):
    """img_crop's (y1, x1, ch, cw): shape clamped into the slice, then min(max(c - half, 0), extent - shape)."""
    ch, cw = min(max(int(crop_hw[0]), 1), src_hw[0]), min(max(int(crop_hw[1]), 1), src_hw[1])
    y1 = min(max(int(center_yx[0]) - ch // 2, 0), src_hw[0] - ch)
    x1 = min(max(int(center_yx[1]) - cw // 2, 0), src_hw[1] - cw)
    return y1, x1, ch, cw


def img_crop(im, cz, channels, box):
    """float64 [C, ch, cw] = stored / IM_SCALE of slices cz - C/2 .. cz + C/2; a slice outside the case is zeros (np.pad)."""
    y1, x1, ch, cw = box
    out = np.zeros((channels, ch, cw), np.float64)
    for c in range(channels):
        z = cz - channels // 2 + c
        if 0 <= z < im.shape[0]:
            out[c] = im[z, y1:y1 + ch, x1:x1 + cw].astype(np.float64) / IM_SCALE
    return out


def object_crop(lab, cz, box, obj_label):
    """The object mask at source resolution, uint8 [ch, cw]: lab_patch of gen_batch :624 with the object as the class."""
    y1, x1, ch, cw = box
    if not 0 <= cz < lab.shape[0]:
        return np.zeros((ch, cw), np.uint8)
    return (lab[cz, y1:y1 + ch, x1:x1 + cw] >= obj_label).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- images and labels
def sample(im, lab, center, crop_hw, shape, flips=(0, 0), gamma=None, obj_label=1):
    """One sample: (image float64 [H, W, C], label int64 [H, W] in {0, 1}, m, s); center = (cz, cy, cx), shape = (C, H, W),
    flips = (left/right, up/down)."""
    c, h, w = shape
    box = crop_box(center[1:], crop_hw, im.shape[1:])
    z, m, s = zscore(img_crop(im, int(center[0]), c, box))
    f3 = (flips[0], flips[1], 0)
    out = lits3d_ref.flip(resize_bilinear(z, (h, w)), f3)
    lb = lits3d_ref.flip(resize_nearest(object_crop(lab, int(center[0]), box, obj_label)[None].astype(np.int64), (h, w)), f3)[0]
    out = np.ascontiguousarray(out.transpose(1, 2, 0))
    if gamma is not None:
        out = augment_gamma(out, float(gamma))
    return out, np.ascontiguousarray(lb), m, s


def noise(seed, shape, scale):
    """float32 [N, H, W, C]: (2 u - 1) * scale with u = unetk_uniform(seed, flat element index), every operation in float32."""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    u = unetk_rng.fc_uniform_host(int(seed) & 0xFFFFFFFF, idx).reshape(shape)
    t = (np.float32(2) * u - np.float32(1)).astype(np.float32)
    return (t * np.float32(scale)).astype(np.float32)


def noise_and_mask(images32, seed, scale):
    """data_processing :521-524 on a float32 batch [N, H, W, C]: add the noise, then multiply every channel by
    float(max over (H, W) of the noised channel > 0)."""
    v = (images32.astype(np.float32) + noise(seed, images32.shape, scale)).astype(np.float32)
    keep = (v.max(axis=(1, 2)) > 0).astype(np.float32)
    return v * keep[:, None, None, :], keep


# ------------------------------------------------------------------------------------------------- clicks
def candidates(mask, margin, band, bg):
    """inter_simulation :379-381: G before the `small` fall-back."""
    g = binary_erosion(mask.astype(bool), iterations=margin, border_value=int(bg))
    if bg:
        g = g ^ binary_erosion(g, iterations=band, border_value=int(bg))
    return g


def inter_simulation(mask, margin, step, n, draws, bg, band, strategy, trace=None):
    """inter_simulation :346-412 with explicit draws: click k of a random choice takes rank (draws[k] * count) >> 32.
    Deviation: a mask without a pixel gives no click (the reference fails converting NaN).  trace (a dict) collects what
    the tests assert about their inputs: small, ranks, counts, ties, emptied."""
    trace = {} if trace is None else trace
    trace.update(small=False, ranks=[], counts=[], ties=0, emptied=False, band_cut=False)
    mask = mask.astype(bool)
    pts = []
    if not mask.any():
        return pts
    g = candidates(mask, margin, band, bg)
    small = not g.max()
    if small:
        g = mask.copy()
    trace["small"] = small
    if bg and not small:                                      # does the crop border cut the band?
        trace["band_cut"] = bool(g[0].any() or g[-1].any() or g[:, 0].any() or g[:, -1].any())
    h, w = mask.shape
    for k in range(n):
        cy, cx = np.where(g)
        if not small:
            if k == 0 or strategy in (0, 1):
                i = (int(draws[k]) * len(cy)) >> 32
                trace["ranks"].append(i)
                trace["counts"].append(len(cy))
            else:
                d = np.stack([cy, cx], axis=1).reshape(-1, 1, 2).astype(np.int64) - np.asarray(pts, np.int64).reshape(1, -1, 2)
                score = np.sum(d ** 2, axis=-1).min(axis=1)
                i = int(np.argmax(score))
                trace["ties"] += int((score == score[i]).sum() > 1)
            y, x = int(cy[i]), int(cx[i])
        else:
            y, x = int(cy.sum()) // len(cy), int(cx.sum()) // len(cx)
        pts.append((y, x))
        y1, y2, x1, x2 = max(y - step, 0), min(y + step + 1, h), max(x - step, 0), min(x + step + 1, w)
        yy, xx = np.meshgrid(np.arange(y1, y2), np.arange(x1, x2), indexing="ij", sparse=True)
        g[y1:y2, x1:x2] &= (xx - x) ** 2 + (yy - y) ** 2 > step ** 2
        if small or not g.max():
            trace["emptied"] = (not small) and k + 1 < n
            break
    return pts


def clicks(obj, row, params=(3, 10, 40, 5), trace=None):
    """gen_kernel :530-561 for one sample: obj uint8 [ch, cw], row = the sample's click_tab row -> (pts int32 [2, 4, 2] with -1
    padding, cnt int32 [2])."""
    margin, step, band, _ = params
    trace = {} if trace is None else trace
    trace["fg"], trace["bg"] = {}, {}
    fg = []
    if obj.max() > 0:
        fg = inter_simulation(obj, margin, step, int(row[0]), row[4:8], False, band, 1, trace["fg"])
    bg = inter_simulation(1 - obj, margin, step, int(row[1]), row[8:12], True, band, int(row[2]), trace["bg"])
    pts = np.full((2, MAX_CLICKS, 2), -1, np.int32)
    for kind, p in enumerate((fg, bg)):
        if p:
            pts[kind, :len(p)] = np.asarray(p, np.int32)
    return pts, np.array([len(fg), len(bg)], np.int32)


def erode_brute(mask, iterations, border):
    """binary_erosion with the cross, one sweep per iteration, pixel by pixel: the check of `candidates`."""
    cur = mask.astype(bool)
    h, w = cur.shape
    for _ in range(iterations):
        nxt = np.zeros_like(cur)
        for y in range(h):
            for x in range(w):
                keep = cur[y, x]
                for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    yy, xx = y + dy, x + dx
                    keep = keep and (cur[yy, xx] if 0 <= yy < h and 0 <= xx < w else bool(border))
                nxt[y, x] = keep
        cur = nxt
    return cur


# ------------------------------------------------------------------------------------------------- guide
def guide_crop(ch, cw, pts, stddev=None):
    """create_spatial_guide_2d on the crop, float64 [ch, cw]: no clicks -> zeros (false_fn)."""
    if len(pts) == 0:
        return np.zeros((ch, cw), np.float64)
    yy, xx = np.meshgrid(np.arange(ch, dtype=np.float64), np.arange(cw, dtype=np.float64), indexing="ij")
    p = np.asarray(pts, np.float64)
    dy2 = (yy[None] - p[:, 0, None, None]) ** 2
    dx2 = (xx[None] - p[:, 1, None, None]) ** 2
    if stddev is None:
        return np.sqrt(dy2 + dx2).min(axis=0)
    return np.exp(-(dy2 / (2. * stddev * stddev) + dx2 / (2. * stddev * stddev))).max(axis=0)


def sp_guide(crop_hw, out_hw, pts, cnt, flips=(0, 0), stddev=None, channels=2):
    """float64 [H, W, channels] and the largest corner distance: both kinds rendered on the crop, resized, flipped."""
    ch, cw = crop_hw
    g = np.stack([guide_crop(ch, cw, [tuple(q) for q in pts[k, :cnt[k]]], stddev) for k in range(2)])
    out = lits3d_ref.flip(resize_bilinear(g, out_hw), (flips[0], flips[1], 0)).transpose(1, 2, 0)
    if channels == 1:
        out = out[..., :1] - out[..., 1:]
    return np.ascontiguousarray(out), float(g.max())
