"""Helpers of the hard-negative tests (test_hard_neg_host.py, test_gpu_hard_neg.py): numpy / scipy restatements of what
`unetk_fp_mask3d`, `unetk_lits3d_clicks_neg` and `PatchSampler.draw_hard_neg` compute, and the inputs of
the reference-pinned click records (tests/golden/ref_clicks3d_neg.json; no GPU code, no RNG).

  mining   DataLoader/NF/input_pipeline_3d.py:187-219 load_neg with scipy.ndimage.label and generate_binary_structure(3, 1),
           literally; the two stated deviations: the overlap is tested against the object class, and min_size is a parameter
  clicks   :258-324 inter_simulation(strategy=4, neg_patch) as :486-504 gen_kernel calls it under cfg.fp_sample, np.random
           replaced by explicit draws as lits3d_clicks_ref does it; test_hard_neg_host.py holds it to what the reference gave
  locate   :595-596 neg_data[pid]["pos"][i]: the i-th voxel of np.where(mask) in (z, y, x) order, as (slice, rank in the slice)
"""
import numpy as np
from scipy.ndimage import find_objects, generate_binary_structure, label

import click3d_shapes as c3
import lits3d_clicks_ref as cref
import lits3d_ref

LAST = c3.LAST


# ------------------------------------------------------------------------------------------------- mining
def fp_mask(pred, lab, pred_label, obj_label, min_size=6, out_value=1):
    """load_neg :207-218 for one case: pred, lab uint8 [D, H, W] with lab in {0, 1, 2} -> (out uint8, slice_counts int64 [D],
    head = [components, kept components, kept voxels, 0])."""
    res, n_obj = label(pred >= pred_label, generate_binary_structure(3, 1))
    obj = lab >= obj_label
    kept = 0
    for i, sli in enumerate(find_objects(res)):
        cube = res[sli]
        if ((cube == i + 1) * obj[sli]).sum() or (cube == i + 1).sum() < min_size:
            cube[cube == i + 1] = 0
        else:
            kept += 1
    mask = np.clip(res, 0, 1).astype(np.uint8)
    counts = mask.sum(axis=(1, 2)).astype(np.int64)
    return mask * np.uint8(out_value), counts, [int(n_obj), kept, int(counts.sum()), 0]


# ------------------------------------------------------------------------------------------------- sampler
def locate(mask, rank):
    """(z, k): the slice of voxel `rank` of np.where(mask) and its rank among the voxels of that slice."""
    z = np.where(mask)[0]
    return int(z[rank]), int(rank - np.searchsorted(z, z[rank], side="left"))


# ------------------------------------------------------------------------------------------------- clicks
def neg_patch(neg, center, crop_hw, shape):
    """uint8 [D, ch, cw]: the false positives under unetk_lits_patch3d's crop box; neg uint8 [depth, src_h, src_w] in {0, 1}.
    Crop slices at or beyond the case's depth hold none."""
    box = lits3d_ref.crop_box(center, crop_hw, shape, neg.shape[0], neg.shape[1:])
    _, lb = lits3d_ref.crop(np.zeros(neg.shape, np.uint16), neg, box, int(shape[0]))
    return (lb > 0).astype(np.uint8)


def strategy4(neg, step, n, draws, trace=None):
    """inter_simulation :287-288, :300-322 with strategy 4: G = neg_patch, every click a random choice among np.where(G) --
    rank (draws[k] * count) >> 32 in (z, y, x) order; after a click its own slice loses the disc of radius step; stops when G
    is empty.  No erosion, no `small`."""
    trace = {} if trace is None else trace
    trace.update(small=False, ranks=[], counts=[], emptied=False)
    g = neg.astype(bool).copy()
    _, h, w = g.shape
    pts = []
    for k in range(n):
        cz, cy, cx = np.where(g)
        i = (int(draws[k]) * len(cz)) >> 32
        trace["ranks"].append(i)
        trace["counts"].append(len(cz))
        z, y, x = int(cz[i]), int(cy[i]), int(cx[i])
        pts.append((z, y, x))
        y1, y2, x1, x2 = max(y - step, 0), min(y + step + 1, h), max(x - step, 0), min(x + step + 1, w)
        yy, xx = np.meshgrid(np.arange(y1, y2), np.arange(x1, x2), indexing="ij", sparse=True)
        g[z, y1:y2, x1:x2] &= (xx - x) ** 2 + (yy - y) ** 2 > step ** 2
        if not g.max():
            trace["emptied"] = k + 1 < n
            break
    return pts


def clicks(obj, neg, row, params=(3, 10, 40, 5), trace=None):
    """gen_kernel :486-504 with cfg.fp_sample for one sample: obj, neg uint8 [D, ch, cw], row = the click_tab row -> (pts int32
    [2, 4, 3] with -1 padding, cnt int32 [2]).  A patch without a false positive is lits3d_clicks_ref.clicks."""
    if not neg.any():
        return cref.clicks(obj, row, params, trace)
    margin, step, band, _ = params
    trace = {} if trace is None else trace
    trace["fg"], trace["bg"] = {}, {}
    fg = []
    if obj.max() > 0:
        fg = cref.inter_simulation(obj, margin, step, int(row[0]), row[4:8], False, band, 1, trace["fg"])
    bg = strategy4(neg, step, int(row[1]), row[8:12], trace["bg"])
    pts = np.full((2, cref.MAX_CLICKS, 3), -1, np.int32)
    for kind, p in enumerate((fg, bg)):
        if p:
            pts[kind, :len(p)] = np.asarray(p, np.int32)
    return pts, np.array([len(fg), len(bg)], np.int32)


# ------------------------------------------------------------------------------------------------- the records' inputs
# Small false-positive masks on the volumes of click3d_shapes: name -> (volume, [(z, y0, x0, y1, x1)] filled rectangles in CASE
# coordinates, y1 / x1 exclusive).  The crop of the "multi" sample on v100 is z 1..6, y 4..99, x 4..103; of "shallow" z 0..5
# (the case has 4 slices), y 2..37, x 2..45.
NEG_MASKS = {
    # one slice, wider than the suppression disc: four clicks fit.  Lies on background far from the object
    "one_slice": ("v100", [(3, 8, 60, 40, 100)]),
    # three slices, one rectangle across the object of slice 4: the label does not matter, (z, y, x) rank order does
    "several": ("v100", [(2, 70, 8, 90, 40), (4, 30, 30, 62, 70), (6, 10, 50, 16, 90)]),
    # 5 x 5 voxels: the first click's disc (radius 10) takes all of it, the kind stops at one click
    "blob": ("v100", [(5, 80, 80, 85, 85)]),
    # only outside the crop box: slice 0 and 7 (the crop takes 1..6) and rows / columns below 4
    "outside": ("v100", [(0, 20, 20, 60, 60), (7, 20, 20, 60, 60), (3, 0, 0, 4, 104), (3, 0, 0, 100, 4)]),
    # the shallow case itself has none: what the crop's two padding slices would cover belongs to the NEXT case of a store
    "shallow_none": ("shallow4", []),
}
# the false positives of the case that follows "shallow4" in the GPU test's store, on ITS first two slices = the crop's padding
SHALLOW_NEXT = [(0, 4, 4, 30, 40), (1, 4, 4, 30, 40)]


def build_neg(name):
    """uint8 [depth, H, W] in {0, 1} of NEG_MASKS[name]."""
    vname, rects = NEG_MASKS[name]
    shape, slices = c3.VOLUMES[vname]
    return rect_volume((len(slices),) + tuple(shape), rects)


def rect_volume(shape, rects):
    out = np.zeros(shape, np.uint8)
    for z, y0, x0, y1, x1 in rects:
        out[z, y0:y1, x0:x1] = 1
    return out


# false positives of the four cases of lits3d_ref.make_cases (depths 12, 9, 5, 9 of 40 x 48): case 0 on three slices, two of
# them neighbours; the tumour-free case 1 on one; the shallow case 2 has none; case 3 on its first and last slice
STORE_NEG = ([(2, 3, 5, 9, 13), (3, 20, 30, 26, 47), (9, 30, 2, 39, 10)], [(4, 10, 10, 16, 16)], [],
             [(0, 0, 0, 4, 6), (8, 33, 40, 40, 48)])


def store_neg():
    """[uint8 [depth, 40, 48] in {0, 1}] for the cases of lits3d_ref.make_cases, in order."""
    return [rect_volume((d, lits3d_ref.H, lits3d_ref.W), rects) for d, rects in zip(lits3d_ref.DEPTHS, STORE_NEG)]


_FG = [0, LAST, 1 << 31, 12345]
_BG = [1 << 31, 0, LAST, 3 << 30]


def _rows(n_bg=4, bg=_BG):
    return [[4, n_bg, strategy, 0] + _FG + list(bg) for strategy in (1, 3)]


# id, neg mask, centre (cz, cy, cx), patch depth D, crop (ch, cw), parameters, click_tab rows; "same_as" = the id of the record
# of click3d_shapes.RECORDS whose clicks a crop without false positives must reproduce
RECORDS = [
    ("one_slice", "one_slice", (4, 90, 95), 6, (96, 100), c3.REF_CLICKS, _rows(), None),
    ("several", "several", (4, 90, 95), 6, (96, 100), c3.REF_CLICKS, _rows(bg=[LAST, 0, 1 << 31, 7 << 29]), None),
    ("several_small", "several", (4, 90, 95), 6, (96, 100), c3.SMALL_CLICKS, _rows(), None),
    ("blob", "blob", (4, 90, 95), 6, (96, 100), c3.REF_CLICKS, _rows(), None),
    ("n_bg0", "one_slice", (4, 90, 95), 6, (96, 100), c3.REF_CLICKS, _rows(n_bg=0), None),
    ("shallow", "shallow_none", (2, 20, 24), 6, (36, 44), c3.REF_CLICKS, c3._rows(), "shallow"),
    ("outside", "outside", (4, 90, 95), 6, (96, 100), c3.REF_CLICKS, c3._rows(fg=[0, c3.FG_NEAR_DRAW, LAST, 12345]), "multi"),
]
