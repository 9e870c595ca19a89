"""Helpers of the elastic deformation tests (test_lits3d_deform_host.py, test_gpu_lits3d_deform.py): the numpy restatement of what
`unetk_lits_patch3d_warp` and `unetk_click_guide3d_warp` compute for a deformed table row.  Builder-written:
the reference has no deformation.  It is built on lits3d_rotate_ref.py (taps, labels, guide) and changes nothing there.

The displacement and the source coordinates are float32, formed in exactly the kernels' operation order with every operation
rounded on its own, so both sides round the SAME numbers to labels; lerps, z-score and the guide are float64.  `displacement64`
is the same spline in float64 at arbitrary real positions, for the folding test."""
import numpy as np

import lits3d_ref as ref
import lits3d_rotate_ref as rref

f32 = np.float32
COL_WARP = 15
FOLD_CAP = 0.4


def cap(out_hw, grid):
    """The largest control displacement `check_values` admits: 0.4 of the control spacing."""
    return FOLD_CAP * (min(out_hw) - 1) / grid


def lattice(rng, px, grid, n=None):
    """Control displacements as the sampler draws them: U(-px, px) in float64, cast to float32, [n, 2, G + 3, G + 3]."""
    shape = (2, grid + 3, grid + 3) if n is None else (n, 2, grid + 3, grid + 3)
    return rng.uniform(-px, px, shape).astype(f32)


def table_row(base, depth, center, crop_hw, flips=(0, 0, 0), gamma=1.0, sc=None, warp=1):
    """lits3d_rotate_ref.table_row with column 15 = warp."""
    row = rref.table_row(base, depth, center, crop_hw, flips, gamma, sc)
    row[COL_WARP] = warp
    return row


def _spline(extent, grid):
    """(cell int [extent], weights float32 [4, extent]) of every output index of one axis."""
    g = f32(f32(grid) / f32(extent - 1)) if extent > 1 else f32(0)
    t = (np.arange(extent, dtype=f32) * g).astype(f32)
    i = np.minimum(np.floor(t).astype(np.int64), grid - 1)
    f = (t - i.astype(f32)).astype(f32)
    r, k6 = (f32(1) - f).astype(f32), f32(1) / f32(6)

    def m(a, b):
        return (a * b).astype(f32)

    def a_(a, b):
        return (a + b).astype(f32)
    w0 = m(m(m(r, r), r), k6)
    w1 = m(a_(m(m(a_(m(f32(3), f), f32(-6)), f), f), f32(4)), k6)
    w2 = m(a_(m(a_(m(a_(m(f32(-3), f), f32(3)), f), f32(3)), f), f32(1)), k6)
    w3 = m(m(m(f, f), f), k6)
    return i, np.stack([w0, w1, w2, w3])


def displacement(out_hw, lat, grid):
    """(dy, dx) float32 [H, W]: sum_a wy[a] * (sum_b wx[b] * lat[c][i + a][j + b]), both sums left to right from term 0."""
    h, w = out_hw
    lat = np.asarray(lat, dtype=f32)
    assert lat.shape == (2, grid + 3, grid + 3), lat.shape
    (i, wy), (j, wx) = _spline(h, grid), _spline(w, grid)
    out = []
    with np.errstate(all="ignore"):
        for c in range(2):
            acc = None
            for a in range(4):
                inner = None
                for b in range(4):
                    term = (wx[b][None, :] * lat[c][(i + a)[:, None], (j + b)[None, :]]).astype(f32)
                    inner = term if inner is None else (inner + term).astype(f32)
                term = (wy[a][:, None] * inner).astype(f32)
                acc = term if acc is None else (acc + term).astype(f32)
            out.append(acc)
    return out[0], out[1]


def displacement64(y, x, out_hw, lat, grid):
    """The same spline in float64 at real positions y [A, 1], x [1, B] of the output patch (0 .. H - 1, 0 .. W - 1); lat may
    carry leading batch axes, which the result keeps."""
    lat = np.asarray(lat, dtype=np.float64)

    def axis(p, extent):
        t = np.asarray(p, np.float64) * (grid / (extent - 1.0))
        i = np.clip(np.floor(t).astype(np.int64), 0, grid - 1)
        f = t - i
        return i, np.stack([(1 - f) ** 3, 3 * f ** 3 - 6 * f ** 2 + 4, -3 * f ** 3 + 3 * f ** 2 + 3 * f + 1, f ** 3]) / 6.0
    (i, wy), (j, wx) = axis(y, out_hw[0]), axis(x, out_hw[1])
    out = []
    for c in range(2):
        acc = 0.0
        for a in range(4):
            for b in range(4):
                acc = acc + wy[a] * wx[b] * lat[..., c, :, :][..., i + a, j + b]
        out.append(acc)
    return out[0], out[1]


def coords(out_hw, crop_hw, lat, grid, sc=None):
    """(in_y, in_x float32 [H, W], ok bool [H, W]) of the un-flipped patch: (y', x') = (y + dy, x + dx), then the row's own map
    -- the align_corners scale, or with sc = (sin, cos) the sums of lits3d_rotate_ref.coords."""
    (h, w), (ch, cw) = out_hw, crop_hw
    dy, dx = displacement(out_hw, lat, grid)
    hs = f32(f32(ch - 1) / f32(h - 1)) if h > 1 else f32(0)
    ws = f32(f32(cw - 1) / f32(w - 1)) if w > 1 else f32(0)
    with np.errstate(all="ignore"):
        yp = (np.arange(h, dtype=f32)[:, None] + dy).astype(f32)
        xp = (np.arange(w, dtype=f32)[None, :] + dx).astype(f32)
        if sc is None:
            in_y, in_x = (yp * hs).astype(f32), (xp * ws).astype(f32)
        else:
            s, c = f32(sc[0]), f32(sc[1])
            cy0, cx0 = f32(0.5) * f32(ch - 1), f32(0.5) * f32(cw - 1)
            u, v = ((yp * hs).astype(f32) - cy0).astype(f32), ((xp * ws).astype(f32) - cx0).astype(f32)
            in_y = (cy0 + ((c * u).astype(f32) - (s * v).astype(f32)).astype(f32)).astype(f32)
            in_x = (cx0 + ((s * u).astype(f32) + (c * v).astype(f32)).astype(f32)).astype(f32)
        ok = np.isfinite(in_y) & np.isfinite(in_x) & (np.abs(in_y) < rref.LIMIT) & (np.abs(in_x) < rref.LIMIT)
    return in_y, in_x, ok


def patch(im, lab, center, crop_hw, shape, lat, grid, sc=None, flips=(0, 0, 0), gamma=None, lab_max=2, info=None):
    """One deformed sample, as lits3d_rotate_ref.patch: (image float64 [D, H, W], label int64 [D, H, W], m, s); only the
    coordinates differ."""
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
    in_y, in_x, ok = coords(shape[1:], (ch, cw), lat, grid, sc)
    iy, ix, i0, j0, fy, fx = rref._taps(in_y, in_x, ok)
    count = dict(outside=0, beyond=0)

    def tap(i, j):
        yy, xx = y1 + i, x1 + j
        inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw) & ok
        count["outside"] += int((~inside & ok).sum())
        count["beyond"] += int((inside & ((i < 0) | (i >= ch) | (j < 0) | (j >= cw))).sum())
        return np.where(inside[None], zs[:, np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0.0)
    tl, tr, bl, br = tap(i0, j0), tap(i0, j0 + 1), tap(i0 + 1, j0), tap(i0 + 1, j0 + 1)
    top, bot = tl + (tr - tl) * fx[None], bl + (br - bl) * fx[None]
    out = top + (bot - top) * fy[None]
    yy, xx = y1 + rref._roundf(iy), x1 + rref._roundf(ix)
    inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw) & ok
    lb = np.where(inside[None], lbv[:, np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0)
    out, lb = ref.flip(out, flips), np.minimum(ref.flip(lb, flips), lab_max)
    if gamma is not None:
        out = ref.augment_gamma(out, float(gamma))
    if info is not None:
        info.update(count, invalid=int((~ok).sum()))
    return np.ascontiguousarray(out), np.ascontiguousarray(lb), m, s


def sp_guide(crop_shape, out_hw, pts, cnt, lat, grid, sc=None, flips=(0, 0, 0), stddev=None, channels=2, norm=1.0):
    """(float64 [D, H, W, channels], far), as lits3d_rotate_ref.sp_guide at the deformed coordinate."""
    d, ch, cw = crop_shape
    in_y, in_x, ok = coords(out_hw, (ch, cw), lat, grid, sc)
    _, _, i0, j0, fy, fx = rref._taps(in_y, in_x, ok)
    z = np.arange(d)[:, None, None]
    out, far = [], 0.0
    for kind in range(2):
        p = [tuple(q) for q in pts[kind, :cnt[kind]]]
        c = []
        for i, j in ((i0, j0), (i0, j0 + 1), (i0 + 1, j0), (i0 + 1, j0 + 1)):
            g, f = rref.guide_at(p, z, i[None], j[None], stddev, norm)
            c.append(g)
            far = max(far, f)
        top, bot = c[0] + (c[1] - c[0]) * fx[None], c[2] + (c[3] - c[2]) * fx[None]
        out.append(ref.flip(np.where(ok[None], top + (bot - top) * fy[None], 0.0), flips))
    out = np.stack(out, axis=-1)
    if channels == 1:
        out = out[..., :1] - out[..., 1:]
    return np.ascontiguousarray(out), far
