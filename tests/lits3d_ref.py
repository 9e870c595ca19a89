"""Helpers of the LiTS 3-D pipeline tests (test_lits3d_host.py, test_gpu_lits3d.py): a tiny LiTS-like dataset in the
reference's on-disk format and the float64 numpy restatement of what `unetk_lits_patch3d` computes.

TensorFlow does not run here, so the restatement is builder-written ("parity unpinned"); each step cites the
reference lines it restates:
  crop      DataLoader/misc.py:132-143 volume_crop (deviation: a case shallower than D starts at slice 0 and is padded with
            zero slices; the crop is clamped to the slice)
  z-score   DataLoader/NF/input_pipeline_3d.py:354-359 (deviation: an empty mask gives m = s = 0, an all-zero patch)
  resize    :381 resize_bilinear / :401 resize_nearest_neighbor, align_corners=True, per slice; the source coordinates are
            TF's float32 ones (out * scale), the lerps are float64
  flips     utils/image_ops.py:287-314
  gamma     utils/image_ops.py:339-354 augment_gamma(retain_stats=True)
"""
import json

import numpy as np

from boxsegliver_amd import _abi

TAB_COLS = _abi.LITS3D_TAB_COLS           # int32 columns of a sample-table row (include/unetk.h)
IM_SCALE = LB_SCALE = 64
H, W = 40, 48
DEPTHS = (12, 9, 5, 9)
K_FOLDS = "Fold 0:0 1\nFold 1:2 3\n"      # test_fold 1: train on cases 0, 1 and validate on 2, 3
SINGLE_PIXEL = (5, 20, 17)                # case 0: slice 5 holds exactly one tumour pixel
AIR = (slice(0, 20), slice(0, 22))        # case 1: stored value 0 on every slice
FLAT = (slice(22, 40), slice(24, 48))     # case 1: one stored value (6400 = 100.0) on every slice


def make_cases():
    """[(image uint16 [d, 40, 48], label uint8 [d, 40, 48] in {0, 1, 2})]: case 0 has tumour blobs touching two opposite
    corners of the volume and a single-pixel tumour slice, case 1 has no tumour, an air block and a flat block, case 2 is
    shallower than the test depth, case 3 is an ordinary case."""
    rng = np.random.default_rng(11)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = []
    for pid, depth in enumerate(DEPTHS):
        lab = np.zeros((depth, H, W), np.uint8)
        liver = ((yy - 20) / 14.0) ** 2 + ((xx - 22) / 16.0) ** 2 <= 1
        lab[1:depth - 1, liver] = 1
        if pid == 0:
            lab[0:2, 0:3, 0:3] = 2
            lab[depth - 2:, H - 3:, W - 3:] = 2
            lab[SINGLE_PIXEL] = 2
            lab[7, 18:23, 20:26] = 2
        elif pid in (2, 3):
            lab[1:3, 15:20, 18:25] = 2
        hu = rng.normal(40, 35, size=(depth, H, W)) + 70 * (lab > 0) - 50 * (lab == 2)
        hu[:, :, W - 5:] = -400                                  # a strip of air on every case: a mask with a border
        im = ((np.clip(hu, -200, 250) + 200) * IM_SCALE).astype(np.uint16)
        if pid == 1:
            im[(slice(None),) + AIR] = 0
            im[(slice(None),) + FLAT] = 6400
        out.append((im, lab))
    return out


def write_dataset(root, cases=None):
    """png/volume-<pid>/<z>_im.png, _lb.png + meta.json + k_folds.txt under `root`, as data/lits.py reads them."""
    from boxsegliver_amd.data import lits
    cases = make_cases() if cases is None else cases
    meta = []
    for pid, (im, lab) in enumerate(cases):
        d = root / "png" / "volume-{:d}".format(pid)
        d.mkdir(parents=True)
        for z in range(im.shape[0]):
            (d / "{:03d}_im.png".format(z)).write_bytes(lits.png_encode(im[z]))
            (d / "{:03d}_lb.png".format(z)).write_bytes(lits.png_encode((lab[z] * LB_SCALE).astype(np.uint8)))
        tz = [int(z) for z in range(im.shape[0]) if (lab[z] == 2).any()]
        boxes = []
        for z in tz:
            ys, xs = np.nonzero(lab[z] == 2)
            boxes.append([int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1])
        meta.append({"PID": pid, "size": [int(im.shape[0]), H, W], "spacing": [2.5, 0.8, 0.8],
                     "bbox": [1, 6, 6, int(im.shape[0]) - 1, 35, 39], "tumors": "[]", "tumor_areas": [], "tumor_centers": "[]",
                     "tumor_stddevs": "[]", "tumor_slices_from_to": list(range(len(tz) + 1)), "tumor_slices": json.dumps(boxes),
                     "tumor_slices_index": tz,
                     "tumor_slices_centers": json.dumps([[(b[0] + b[2]) / 2., (b[1] + b[3]) / 2.] for b in boxes]),
                     "tumor_slices_stddevs": json.dumps([[2.0, 2.0] for _ in boxes]),
                     "tumor_slices_areas": [int((lab[z] == 2).sum()) for z in tz], "tumor_slices_tid": [0] * len(tz)})
    (root / "meta.json").write_text(json.dumps(meta))
    (root / "k_folds.txt").write_text(K_FOLDS)
    return cases


def stack_store(cases):
    """The resident store of `cases` in order: (im uint16 [n, 40, 48], lb uint8 [n, 40, 48] = label * 64, base [n_cases])."""
    im = np.concatenate([c[0] for c in cases])
    lb = np.concatenate([(c[1] * LB_SCALE).astype(np.uint8) for c in cases])
    base = np.concatenate(([0], np.cumsum([c[0].shape[0] for c in cases])))[:-1]
    return im, lb, base


# ------------------------------------------------------------------------------------------------- the restatement
def crop_box(center, crop_hw, shape, depth, src_hw):
    """volume_crop's (z1, y1, x1, ch, cw) for a D-deep crop around `center` = (cz, cy, cx)."""
    d = int(shape[0])
    ch, cw = min(max(int(crop_hw[0]), 1), src_hw[0]), min(max(int(crop_hw[1]), 1), src_hw[1])
    z1 = min(max(int(center[0]) - d // 2, 0), max(depth - d, 0))
    y1 = min(max(int(center[1]) - ch // 2, 0), src_hw[0] - ch)
    x1 = min(max(int(center[2]) - cw // 2, 0), src_hw[1] - cw)
    return z1, y1, x1, ch, cw


def crop(im, lab, box, d):
    """(image float64 [D, ch, cw] = stored / IM_SCALE, label int64 [D, ch, cw]); slices beyond the case are zeros."""
    z1, y1, x1, ch, cw = box
    img = np.zeros((d, ch, cw), np.float64)
    lb = np.zeros((d, ch, cw), np.int64)
    n = max(min(d, im.shape[0] - z1), 0)
    img[:n] = im[z1:z1 + n, y1:y1 + ch, x1:x1 + cw].astype(np.float64) / IM_SCALE
    lb[:n] = lab[z1:z1 + n, y1:y1 + ch, x1:x1 + cw]
    return img, lb


def zscore(img):
    """data_processing :354-359: (img - region * mean) / (region * sd + 1e-8) over region = img > 0 -> (out, m, s)."""
    region = img > 0
    if region.any():
        vals = img[region]
        m, s = float(vals.mean()), float(np.sqrt(vals.var()))
    else:
        m = s = 0.0                                              # deviation 2: TF's moments of nothing are NaN
    r = region.astype(np.float64)
    return (img - r * m) / (r * s + 1e-8), m, s


def _coords(n_in, n_out):
    scale = np.float32((n_in - 1) / (n_out - 1)) if n_out > 1 else np.float32(0)
    return (np.arange(n_out, dtype=np.float32) * scale).astype(np.float32)      # TF's float32 source coordinates


def resize_bilinear(img, out_hw):
    """resize_bilinear(align_corners=True) of every slice of img [D, h, w]: float32 coordinates, float64 lerps in TF's
    order (along x on both rows, then along y)."""
    _, h, w = img.shape
    ys, xs = _coords(h, out_hw[0]), _coords(w, out_hw[1])
    y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    ly = (ys - y0.astype(np.float32)).astype(np.float64)[None, :, None]
    lx = (xs - x0.astype(np.float32)).astype(np.float64)[None, None, :]
    tl, tr = img[:, y0][:, :, x0], img[:, y0][:, :, x1]
    bl, br = img[:, y1][:, :, x0], img[:, y1][:, :, x1]
    top, bot = tl + (tr - tl) * lx, bl + (br - bl) * lx
    return top + (bot - top) * ly


def resize_nearest(lab, out_hw):
    """resize_nearest_neighbor(align_corners=True): roundf of the float32 coordinate."""
    _, h, w = lab.shape
    ys = np.minimum(np.floor(_coords(h, out_hw[0]).astype(np.float64) + 0.5).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(_coords(w, out_hw[1]).astype(np.float64) + 0.5).astype(np.int64), w - 1)
    return lab[:, ys][:, :, xs]


def flip(a, flips):
    """random_flip's three reversals on [D, H, W]: flips = (left/right, up/down, front/back)."""
    if flips[0]:
        a = a[:, :, ::-1]
    if flips[1]:
        a = a[:, ::-1, :]
    if flips[2]:
        a = a[::-1]
    return a


def augment_gamma(x, gamma, epsilon=1e-7):
    """image_ops.py:339-354 with retain_stats=True, in float64."""
    mn, sd = x.mean(), np.sqrt(x.var())
    minm = x.min()
    rnge = x.max() - minm
    y = np.power((x - minm) / (rnge + epsilon), gamma) * rnge + minm
    new_mn, new_sd = y.mean(), np.sqrt(y.var())
    y = y - new_mn + mn
    return y / (new_sd + 1e-8) * sd


def patch(im, lab, center, crop_hw, shape, flips=(0, 0, 0), gamma=None, lab_max=2):
    """One sample: (image float64 [D, H, W], label int64 [D, H, W], m, s) of case (im uint16, lab uint8 in {0, 1, 2})."""
    box = crop_box(center, crop_hw, shape, im.shape[0], im.shape[1:])
    img, lb = crop(im, lab, box, shape[0])
    z, m, s = zscore(img)
    out = flip(resize_bilinear(z, shape[1:]), flips)
    lb = np.minimum(flip(resize_nearest(lb, shape[1:]), flips), lab_max)
    if gamma is not None:
        out = augment_gamma(out, float(gamma))
    return np.ascontiguousarray(out), np.ascontiguousarray(lb), m, s


def table_row(base, depth, center, crop_hw, flips=(0, 0, 0), gamma=1.0, forced=0, k=0):
    row = np.zeros(TAB_COLS, dtype=np.int32)
    row[0:2] = base, depth
    row[2:5] = center
    row[5:7] = crop_hw
    row[7:10] = flips
    row[10] = np.array([gamma], dtype=np.float32).view(np.int32)[0]
    row[11:13] = forced, k
    return row
