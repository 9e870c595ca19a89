"""Helpers of the 3-D click-guide tests (test_lits3d_clicks_host.py, test_gpu_lits3d_clicks.py): the float64 / integer numpy
restatement of what `unetk_lits3d_clicks` and `unetk_click_guide3d` compute.

`clicks` restates plain numpy / scipy code of the reference that runs in the build container: test_lits3d_clicks_host.py holds
it to what the reference itself gave (tests/golden/ref_clicks3d.json).  The guide is TensorFlow code and is builder-written
("parity unpinned").  Each step cites the reference lines it restates:
  crop       DataLoader/misc.py:132-143 volume_crop as lits3d_ref.crop_box / crop cut it (a shallow case is padded with
             label-0 slices); the object is stored label >= obj_label
  clicks     DataLoader/NF/input_pipeline_3d.py:258-324 inter_simulation as :474-504 gen_kernel calls it, np.random replaced
             by explicit draws; scipy's binary_erosion with the reference's element (:290-291) used literally, so that the
             kernels' distance shortcut is what gets tested
  guide      utils/image_ops.py:437-472 create_spatial_guide_3d, the division of :372, then the resize and the flips of the
             image (lits3d_ref)
"""
import math

import numpy as np
from scipy.ndimage import binary_erosion

import lits3d_ref

MAX_CLICKS = 4
CLICK_TAB_COLS = 12
STRUCT = np.zeros((3, 3, 3), dtype=bool)         # inter_simulation :290-291
STRUCT[1] = True


# ------------------------------------------------------------------------------------------------- crop
def object_patch(lab, center, crop_hw, shape, obj_label):
    """(uint8 [D, ch, cw] in {0, 1}, box): the label patch of unetk_lits_patch3d's crop box at source resolution, object =
    label >= obj_label; lab uint8 [depth, src_h, src_w] in {0, 1, 2}."""
    box = lits3d_ref.crop_box(center, crop_hw, shape, lab.shape[0], lab.shape[1:])
    _, lb = lits3d_ref.crop(np.zeros(lab.shape, np.uint16), lab, box, int(shape[0]))
    return (lb >= obj_label).astype(np.uint8), box


# ------------------------------------------------------------------------------------------------- clicks
def candidates(mask, margin, band, bg):
    """inter_simulation :290-294: G before the `small` fall-back."""
    g = binary_erosion(mask.astype(bool), STRUCT, iterations=margin, border_value=int(bg))
    if bg:
        g = g ^ binary_erosion(g, STRUCT, iterations=band, border_value=int(bg))
    return g


def round_half_even_mean(total, count):
    """np.round(total / count) for integers, in integers."""
    q, r = divmod(int(total), int(count))
    if 2 * r < count:
        return q
    if 2 * r > count:
        return q + 1
    return q + (q & 1)


def inter_simulation(mask, margin, step, n, draws, bg, band, strategy, trace=None):
    """inter_simulation :258-324 with explicit draws: click k of a random choice takes rank (draws[k] * count) >> 32 among
    np.where(G), i.e. in (z, y, x) order.  Deviation: a mask without a voxel gives no click (the reference fails converting
    NaN).  trace (a dict) collects what the tests assert about their inputs."""
    trace = {} if trace is None else trace
    trace.update(small=False, ranks=[], counts=[], ties=0, cross_ties=0, dz_wins=0, emptied=False, half=[])
    mask = mask.astype(bool)
    pts = []
    if not mask.any():
        return pts
    g = candidates(mask, margin, band, bg)
    small = not g.max()
    if small:
        g = mask.copy()
    trace["small"] = small
    _, h, w = mask.shape
    for k in range(n):
        cz, cy, cx = np.where(g)
        if not small:
            if k == 0 or strategy in (0, 1):
                i = (int(draws[k]) * len(cz)) >> 32
                trace["ranks"].append(i)
                trace["counts"].append(len(cz))
            else:
                ctr = np.stack([cz, cy, cx], axis=1).astype(np.int64)
                d = ctr.reshape(-1, 1, 3) - np.asarray(pts, np.int64).reshape(1, -1, 3)
                score = np.sum(d ** 2, axis=-1).min(axis=1)
                i = int(np.argmax(score))
                best = np.flatnonzero(score == score[i])
                trace["ties"] += int(len(best) > 1)
                trace["cross_ties"] += int(len(set(cz[best].tolist())) > 1)
                flat = np.sum(d[..., 1:] ** 2, axis=-1).min(axis=1)                 # the in-plane distance alone
                trace["dz_wins"] += int(int(np.argmax(flat)) != i)
            z, y, x = int(cz[i]), int(cy[i]), int(cx[i])
        else:
            z, y, x = (round_half_even_mean(c.sum(), len(c)) for c in (cz, cy, cx))
            trace["half"] = [(2 * (int(c.sum()) % len(c)) == len(c), (int(c.sum()) // len(c)) & 1) for c in (cz, cy, cx)]
            want = np.stack([cz, cy, cx], axis=1).mean(axis=0).round().astype(np.int32)     # :310, literally
            assert (z, y, x) == tuple(int(v) for v in want)
        pts.append((z, y, x))
        y1, y2, x1, x2 = max(y - step, 0), min(y + step + 1, h), max(x - step, 0), min(x + step + 1, w)
        yy, xx = np.meshgrid(np.arange(y1, y2), np.arange(x1, x2), indexing="ij", sparse=True)
        g[z, y1:y2, x1:x2] &= (xx - x) ** 2 + (yy - y) ** 2 > step ** 2            # :320: the click's own slice only
        if small or not g.max():
            trace["emptied"] = (not small) and k + 1 < n
            break
    return pts


def clicks(obj, row, params=(3, 10, 40, 5), trace=None):
    """gen_kernel :491-504 for one sample: obj uint8 [D, ch, cw], row = the sample's click_tab row -> (pts int32 [2, 4, 3] with
    -1 padding, cnt int32 [2])."""
    margin, step, band, _ = params
    trace = {} if trace is None else trace
    trace["fg"], trace["bg"] = {}, {}
    fg = []
    if obj.max() > 0:
        fg = inter_simulation(obj, margin, step, int(row[0]), row[4:8], False, band, 1, trace["fg"])
    bg = inter_simulation(1 - obj, margin, step, int(row[1]), row[8:12], True, band, int(row[2]), trace["bg"])
    pts = np.full((2, MAX_CLICKS, 3), -1, np.int32)
    for kind, p in enumerate((fg, bg)):
        if p:
            pts[kind, :len(p)] = np.asarray(p, np.int32)
    return pts, np.array([len(fg), len(bg)], np.int32)


def erode_brute(mask, iterations, border):
    """binary_erosion with the 3 x 3 square of one slice, one sweep per iteration, voxel by voxel: the check of `candidates`."""
    cur = mask.astype(bool)
    d, h, w = cur.shape
    for _ in range(iterations):
        nxt = np.zeros_like(cur)
        for z in range(d):
            for y in range(h):
                for x in range(w):
                    keep = True
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xx = y + dy, x + dx
                            keep = keep and (cur[z, yy, xx] if 0 <= yy < h and 0 <= xx < w else bool(border))
                    nxt[z, y, x] = keep
        cur = nxt
    return cur


def chessboard_sets(mask, margin, band, bg):
    """The candidate set as a threshold of the per-slice chessboard distance, computed by brute force over the zeros: what
    the kernels' separable passes must equal (include/unetk.h)."""
    mask = mask.astype(bool)
    d, h, w = mask.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros_like(mask)
    for z in range(d):
        zy, zx = np.where(~mask[z])
        dist = np.full((h, w), 10 ** 6, np.int64)
        if len(zy):
            dist = np.maximum(np.abs(yy[..., None] - zy), np.abs(xx[..., None] - zx)).min(axis=-1)
        if not bg:                                                               # border_value = 0: outside counts as zero
            dist = np.minimum(dist, np.minimum(np.minimum(yy + 1, h - yy), np.minimum(xx + 1, w - xx)))
            out[z] = dist > margin
        else:
            out[z] = (dist > margin) & (dist <= margin + band)
    return out


# ------------------------------------------------------------------------------------------------- guide
def euclid_norm(im_height):
    """data_processing :372: the python float im_height * sqrt(2) * 0.8, which TensorFlow converts to float32."""
    return float(np.float32(int(im_height) * math.sqrt(2) * 0.8))


def guide_crop(shape, pts, stddev=None, norm=1.0):
    """create_spatial_guide_3d on the crop [D, ch, cw], float64: no clicks -> zeros (false_fn).  stddev None: Euclidean,
    divided by norm; else (s_z, s_y, s_x)."""
    if len(pts) == 0:
        return np.zeros(shape, np.float64)
    zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    p = np.asarray(pts, np.float64)
    dz2 = (zz[None] - p[:, 0, None, None, None]) ** 2
    dy2 = (yy[None] - p[:, 1, None, None, None]) ** 2
    dx2 = (xx[None] - p[:, 2, None, None, None]) ** 2
    if stddev is None:
        return np.sqrt(dz2 + dy2 + dx2).min(axis=0) / norm
    sz, sy, sx = (float(v) for v in stddev)
    return np.exp(-(dz2 / (2. * sz * sz) + dy2 / (2. * sy * sy) + dx2 / (2. * sx * sx))).max(axis=0)


def sp_guide(crop_shape, out_hw, pts, cnt, flips=(0, 0, 0), stddev=None, channels=2, norm=1.0):
    """(float64 [D, H, W, channels], the largest un-normalised corner distance): both kinds rendered on the crop, resized per
    slice, flipped on all three axes with the image."""
    g = [guide_crop(crop_shape, [tuple(q) for q in pts[k, :cnt[k]]], stddev, norm) for k in range(2)]
    out = np.stack([lits3d_ref.flip(lits3d_ref.resize_bilinear(v, out_hw), flips) for v in g], axis=-1)
    if channels == 1:
        out = out[..., :1] - out[..., 1:]
    far = max(float(v.max()) for v in g) * (norm if stddev is None else 1.0)
    return np.ascontiguousarray(out), far
