"""Helpers of the in-plane rotation tests (test_lits3d_rotate_host.py, test_gpu_lits3d_rotate.py): the numpy restatement of
what `unetk_lits_patch3d_rot` and `unetk_click_guide3d_rot` compute for a rotated table row.  Builder-written:
the reference has no rotation.  It leans on lits3d_ref.py and lits3d_clicks_ref.py and changes neither.

The source coordinates are float32 and formed in exactly the kernels' operation order, every operation rounded on its own (no
fused multiply-add), so both sides round the SAME numbers to labels; lerps, z-score and the guide are float64; roundf is taken
on the float64 value of the float32 coordinate."""
import numpy as np

import lits3d_clicks_ref as cref
import lits3d_ref as ref

f32 = np.float32
LIMIT = 2.0 ** 24                    # a coordinate at or beyond it (or not finite) counts as outside
COL_SIN, COL_COS = 13, 14


def sincos(deg):
    """(sin, cos) as the sampler forms them: float64, cast to float32."""
    rad = np.deg2rad(np.float64(deg))
    return f32(np.sin(rad)), f32(np.cos(rad))


def bits(v):
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


def table_row(base, depth, center, crop_hw, flips=(0, 0, 0), gamma=1.0, sc=None):
    """lits3d_ref.table_row with sc = (sin, cos) as float bits in columns 13 / 14; None leaves them zero (not rotated)."""
    row = ref.table_row(base, depth, center, crop_hw, flips, gamma)
    if sc is not None:
        row[COL_SIN], row[COL_COS] = bits(sc[0]), bits(sc[1])
    return row


def coords(out_hw, crop_hw, sc):
    """(in_y, in_x float32 [H, W], ok bool [H, W]) of the un-flipped patch."""
    (h, w), (ch, cw) = out_hw, crop_hw
    s, c = f32(sc[0]), f32(sc[1])
    hs = f32(f32(ch - 1) / f32(h - 1)) if h > 1 else f32(0)
    ws = f32(f32(cw - 1) / f32(w - 1)) if w > 1 else f32(0)
    cy0, cx0 = f32(0.5) * f32(ch - 1), f32(0.5) * f32(cw - 1)
    y, x = np.arange(h, dtype=f32)[:, None], np.arange(w, dtype=f32)[None, :]
    with np.errstate(all="ignore"):
        u, v = (y * hs).astype(f32) - cy0, (x * ws).astype(f32) - cx0
        in_y = cy0 + ((c * u).astype(f32) - (s * v).astype(f32)).astype(f32)
        in_x = cx0 + ((s * u).astype(f32) + (c * v).astype(f32)).astype(f32)
        in_y, in_x = in_y.astype(f32), in_x.astype(f32)
        ok = np.isfinite(in_y) & np.isfinite(in_x) & (np.abs(in_y) < LIMIT) & (np.abs(in_x) < LIMIT)
    return in_y, in_x, ok


def _roundf(v):
    """C's roundf (half away from zero) of float32 values, in float64."""
    v = v.astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5)).astype(np.int64)


def _taps(in_y, in_x, ok):
    iy, ix = np.where(ok, in_y, f32(0)), np.where(ok, in_x, f32(0))
    i0, j0 = np.floor(iy).astype(np.int64), np.floor(ix).astype(np.int64)
    fy = (iy - i0.astype(f32)).astype(np.float64)
    fx = (ix - j0.astype(f32)).astype(np.float64)
    return iy, ix, i0, j0, fy, fx


def patch(im, lab, center, crop_hw, shape, sc, flips=(0, 0, 0), gamma=None, lab_max=2, info=None):
    """One rotated sample: (image float64 [D, H, W], label int64 [D, H, W], m, s).  The statistics are those of the
    axis-aligned crop; the taps read the slice.  info (a dict) counts the taps that left the slice (`outside`) and those that
    read beyond the crop box inside the slice (`beyond`)."""
    d = int(shape[0])
    box = ref.crop_box(center, crop_hw, shape, im.shape[0], im.shape[1:])
    z1, y1, x1, ch, cw = box
    _, m, s = ref.zscore(ref.crop(im, lab, box, d)[0])
    sh, sw = im.shape[1:]
    n = max(min(d, im.shape[0] - z1), 0)
    vol, lbv = np.zeros((d, sh, sw), np.float64), np.zeros((d, sh, sw), np.int64)
    vol[:n] = im[z1:z1 + n].astype(np.float64) / ref.IM_SCALE
    lbv[:n] = lab[z1:z1 + n]
    zs = np.where(vol > 0, (vol - m) / (s + 1e-8), 0.0)
    in_y, in_x, ok = coords(shape[1:], (ch, cw), sc)
    iy, ix, i0, j0, fy, fx = _taps(in_y, in_x, ok)
    outside = beyond = 0

    def tap(i, j):
        nonlocal outside, beyond
        yy, xx = y1 + i, x1 + j
        inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw) & ok
        outside += int((~inside & ok).sum())
        beyond += int((inside & ((i < 0) | (i >= ch) | (j < 0) | (j >= cw))).sum())
        return np.where(inside[None], zs[:, np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0.0)
    tl, tr, bl, br = tap(i0, j0), tap(i0, j0 + 1), tap(i0 + 1, j0), tap(i0 + 1, j0 + 1)
    top, bot = tl + (tr - tl) * fx[None], bl + (br - bl) * fx[None]
    out = top + (bot - top) * fy[None]
    yy, xx = y1 + _roundf(iy), x1 + _roundf(ix)
    inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw) & ok
    lb = np.where(inside[None], lbv[:, np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0)
    out, lb = ref.flip(out, flips), np.minimum(ref.flip(lb, flips), lab_max)
    if gamma is not None:
        out = ref.augment_gamma(out, float(gamma))
    if info is not None:
        info.update(outside=outside, beyond=beyond, invalid=int((~ok).sum()))
    return np.ascontiguousarray(out), np.ascontiguousarray(lb), m, s


def guide_at(pts, z, y, x, stddev=None, norm=1.0):
    """create_spatial_guide_3d (lits3d_clicks_ref.guide_crop) at arbitrary integer positions z [D, 1, 1], y, x [1, H, W], float64:
    -> (guide [D, H, W], the largest un-normalised distance)."""
    shape = np.broadcast(z, y, x).shape
    if len(pts) == 0:
        return np.zeros(shape, np.float64), 0.0
    p = np.asarray(pts, np.float64)
    dz2 = (z[None].astype(np.float64) - p[:, 0, None, None, None]) ** 2
    dy2 = (y[None].astype(np.float64) - p[:, 1, None, None, None]) ** 2
    dx2 = (x[None].astype(np.float64) - p[:, 2, None, None, None]) ** 2
    dist = np.sqrt(dz2 + dy2 + dx2).min(axis=0)
    if stddev is None:
        return dist / norm, float(dist.max())
    sz, sy, sx = (float(v) for v in stddev)
    return np.exp(-(dz2 / (2. * sz * sz) + dy2 / (2. * sy * sy) + dx2 / (2. * sx * sx))).max(axis=0), float(dist.max())


def sp_guide(crop_shape, out_hw, pts, cnt, sc, flips=(0, 0, 0), stddev=None, channels=2, norm=1.0):
    """(float64 [D, H, W, channels], far): both kinds evaluated at the four unclamped corners of the rotated coordinate and
    lerped; 0 where the coordinate is invalid.  far: the largest un-normalised corner distance over the corners visited."""
    d, ch, cw = crop_shape
    in_y, in_x, ok = coords(out_hw, (ch, cw), sc)
    _, _, i0, j0, fy, fx = _taps(in_y, in_x, ok)
    z = np.arange(d)[:, None, None]
    out, far = [], 0.0
    for kind in range(2):
        p = [tuple(q) for q in pts[kind, :cnt[kind]]]
        c = []
        for i, j in ((i0, j0), (i0, j0 + 1), (i0 + 1, j0), (i0 + 1, j0 + 1)):
            g, f = guide_at(p, z, i[None], j[None], stddev, norm)
            c.append(g)
            far = max(far, f)
        top, bot = c[0] + (c[1] - c[0]) * fx[None], c[2] + (c[3] - c[2]) * fx[None]
        out.append(ref.flip(np.where(ok[None], top + (bot - top) * fy[None], 0.0), flips))
    out = np.stack(out, axis=-1)
    if channels == 1:
        out = out[..., :1] - out[..., 1:]
    return np.ascontiguousarray(out), far
