"""GPU: elastically deformed LiTS 3-D patches and their click guides (`unetk_lits_patch3d_warp`, `unetk_click_guide3d_warp`;
csrc/lits3d.hip, csrc/lits3d_clicks.hip, csrc/lits_geom.h): rows that are not deformed against the `_rot` and
plain entries bit for bit, constant lattices against the plain entry of the shifted crop, general lattices against the
restatement (lits3d_deform_ref.py), hostile lattices and table contents inside guard bands, and `liver_3d --random_deform`
training UNet3D from the command line."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import guardbuf
import lits3d_clicks_ref as cref
import lits3d_deform_ref as dref
import lits3d_ref as ref
import lits3d_rotate_ref as rref
from test_gpu_lits3d import GAMMA_MAX_DEV_MEASURED, _samples
from test_gpu_lits3d_clicks import GAUSS_MAX_DEV_MEASURED, _guide_inputs

pytestmark = pytest.mark.gpu

SMALL, LARGE, SQUARE = (6, 16, 20), (6, 32, 40), (6, 16, 16)
ANGLES = (None, 17.0, 45.0)
FLIPS = [(i & 1, (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]


@pytest.fixture(scope="module")
def store():
    cases = ref.make_cases()
    im, lb, base = ref.stack_store(cases)
    return dict(cases=cases, base=base, im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy(lb).cuda())


def _sc(angle):
    return None if angle is None else rref.sincos(angle)


def _table(store, rows, gammas=None):
    """rows: (case, centre, crop, flips, (sin, cos) or None, column 15)."""
    out = [dref.table_row(store["base"][ci], ref.DEPTHS[ci], c, crop, flips, 1.0 if gammas is None else gammas[j], sc, warp)
           for j, (ci, c, crop, flips, sc, warp) in enumerate(rows)]
    return torch.from_numpy(np.stack(out)).cuda()


def _run(store, tab, shape, lat=None, grid=0, training=False, lab_max=2, rotate=False):
    """lat None: the _rot entry (rotate) or the plain one; else the _warp entry."""
    from boxsegliver_amd import ops
    warp = None if lat is None else torch.from_numpy(np.ascontiguousarray(lat, dtype=np.float32)).cuda()
    images, labels = ops.lits_patch3d(store["im"], store["lb"], tab, shape, training, lab_max, rotate=rotate, warp=warp, grid=grid)
    assert images.shape == (tab.shape[0],) + tuple(shape) + (1,) and images.dtype == torch.float32
    assert labels.shape == (tab.shape[0],) + tuple(shape) and labels.dtype == torch.int32
    return images[..., 0].cpu().numpy(), labels.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _lattices(n, shape, grid, seed, quarter_every=0):
    """n lattices at the cap of `shape`; every quarter_every-th (odd rows for 2) at a quarter of it."""
    px = dref.cap(shape[1:], grid)
    rng = np.random.default_rng(seed)
    lat = np.stack([dref.lattice(rng, px / 4 if quarter_every and j % quarter_every == 1 else px, grid) for j in range(n)])
    return lat, px


# ------------------------------------------------------------------------------------------------- 1. rows that are not deformed
@pytest.mark.parametrize("training", [False, True])
def test_rows_that_are_not_deformed_are_the_rot_entry_bit_for_bit(store, training):
    grid = 4
    samples = _samples(LARGE, 1.4) + _samples(LARGE, 1.125)[:5]
    rows = [(ci, c, crop, f, _sc((None, 17.0, None, -33.0)[j % 4]), (0, 0, 1, 7)[(j // 2) % 4])
            for j, (ci, c, crop, f) in enumerate(samples)]
    assert {(r[4] is None, r[5] == 0) for r in rows} == {(a, b) for a in (False, True) for b in (False, True)}
    gammas = [0.7 + 0.03 * j for j in range(len(rows))]
    lat, _ = _lattices(len(rows), LARGE, grid, 21)
    tab = _table(store, rows, gammas)
    got = _run(store, tab, LARGE, lat, grid, training)
    rot = _run(store, tab, LARGE, training=training, rotate=True)                      # the _rot entry ignores column 15
    plain = _run(store, tab, LARGE, training=training)                                 # the plain entry columns 13 .. 15
    for j, row in enumerate(rows):
        same = np.array_equal(_bits(got[0][j]), _bits(rot[0][j])) and np.array_equal(got[1][j], rot[1][j])
        assert same == (row[5] == 0), (j, row)
        if row[4] is None and row[5] == 0:
            assert np.array_equal(_bits(got[0][j]), _bits(plain[0][j])) and np.array_equal(got[1][j], plain[1][j]), j
    # an all-zero column through the _warp entry is the _rot batch, and with columns 13 / 14 zero too the plain batch;
    # the lattices of such rows are never read, whatever they hold
    bad = np.full_like(lat, np.nan)
    zero = _table(store, [r[:5] + (0,) for r in rows], gammas)
    a = _run(store, zero, LARGE, bad, grid, training)
    assert np.array_equal(_bits(a[0]), _bits(rot[0])) and np.array_equal(a[1], rot[1])
    zero = _table(store, [r[:4] + (None, 0) for r in rows], gammas)
    a, b = _run(store, zero, LARGE, bad, grid, training), _run(store, zero, LARGE, training=training)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0)])
def test_guide_rows_that_are_not_deformed_are_the_rot_entry_bit_for_bit(store, stddev):
    from boxsegliver_amd import ops
    grid = 3
    samples, pts, cnt = _guide_inputs(LARGE)
    keep = [0, 1, 2, 3, 4, 0, 1, 3, 2, 3, 1, 0]
    rows = [samples[i] + (_sc((None, 17.0, None, -33.0)[j % 4]), (0, 0, 1, -5)[(j // 2) % 4]) for j, i in enumerate(keep)]
    assert {(r[4] is None, r[5] == 0) for r in rows} == {(a, b) for a in (False, True) for b in (False, True)}
    tab = _table(store, rows)
    lat, _ = _lattices(len(rows), LARGE, grid, 22)
    warp = torch.from_numpy(lat).cuda()
    dp, dc = torch.from_numpy(pts[keep]).cuda(), torch.from_numpy(cnt[keep]).cuda()
    for g in (1, 2):
        got = ops.click_guide3d(tab, dp, dc, LARGE, (ref.H, ref.W), g, stddev, warp=warp, grid=grid).cpu().numpy()
        rot = ops.click_guide3d(tab, dp, dc, LARGE, (ref.H, ref.W), g, stddev, rotate=True).cpu().numpy()
        plain = ops.click_guide3d(tab, dp, dc, LARGE, (ref.H, ref.W), g, stddev).cpu().numpy()
        for j, i in enumerate(keep):
            same = np.array_equal(_bits(got[j]), _bits(rot[j]))
            assert same == (rows[j][5] == 0 or cnt[i].sum() == 0), (g, j)                # sample 4 has no click: all zeros
            if rows[j][4] is None and rows[j][5] == 0:
                assert np.array_equal(_bits(got[j]), _bits(plain[j])), (g, j)
        zero = _table(store, [r[:4] + (None, 0) for r in rows])
        a = ops.click_guide3d(zero, dp, dc, LARGE, (ref.H, ref.W), g, stddev, warp=torch.full_like(warp, float("nan")), grid=grid)
        b = ops.click_guide3d(zero, dp, dc, LARGE, (ref.H, ref.W), g, stddev)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------- 2. integer shifts
@pytest.mark.parametrize("grid", [1, 3])
def test_constant_lattice_is_the_plain_labels_of_the_shifted_crop(store, grid):
    """Square crop at zoom 1: a lattice constant at (dy, dx) moves every coordinate by that many pixels up to a few ulp, so the
    labels are exactly those of the crop moved by the shift -- the plain entry's where the moved crop stays inside the slice, and
    0 where it leaves it -- under all eight flips."""
    crop = SQUARE[1:]
    places = [(0, (6, 19, 23)), (0, (0, 0, 0)), (0, (11, 39, 47)), (2, (2, 17, 21)), (3, (5, 20, 40))]
    shifts = [(2, -3), (-1, 4)]
    rows = [(ci, c, crop, f, None, 1) for ci, c in places for f in FLIPS for _ in shifts]
    lat = np.empty((len(rows), 2, grid + 3, grid + 3), np.float32)
    for j in range(len(rows)):
        lat[j, 0], lat[j, 1] = shifts[j % 2]
    lab = _run(store, _table(store, rows), SQUARE, lat, grid)[1]
    inside = zeros = 0
    j = 0
    for ci, c in places:
        _, lb = store["cases"][ci]
        z1, y1, x1, ch, cw = ref.crop_box(c, crop, SQUARE, ref.DEPTHS[ci], (ref.H, ref.W))
        for f in FLIPS:
            for dy, dx in shifts:
                want = np.zeros(SQUARE, np.int64)
                n = max(min(SQUARE[0], lb.shape[0] - z1), 0)
                ys, xs = y1 + dy + np.arange(ch), x1 + dx + np.arange(cw)
                oky, okx = (ys >= 0) & (ys < ref.H), (xs >= 0) & (xs < ref.W)
                want[:n][:, oky[:, None] & okx[None, :]] = lb[z1:z1 + n][:, ys[oky]][:, :, xs[okx]].reshape(n, -1)
                np.testing.assert_array_equal(lab[j], ref.flip(want, f), err_msg=str((ci, c, f, dy, dx)))
                zeros += int((~oky).sum() + (~okx).sum())
                if oky.all() and okx.all():                                            # the moved crop is a crop: the plain entry cuts it
                    moved = (c[0], y1 + dy + ch // 2, x1 + dx + cw // 2)
                    assert ref.crop_box(moved, crop, SQUARE, ref.DEPTHS[ci], (ref.H, ref.W)) == (z1, y1 + dy, x1 + dx, ch, cw)
                    plain = _run(store, _table(store, [(ci, moved, crop, f, None, 0)]), SQUARE)
                    np.testing.assert_array_equal(lab[j], plain[1][0])
                    inside += 1
                j += 1
    assert inside >= 8 and zeros > 0 and {int(v) for v in np.unique(lab)} == {0, 1, 2}


# ------------------------------------------------------------------------------------------------- 3. general lattices
@pytest.mark.parametrize("grid", [1, 3, 4])
@pytest.mark.parametrize("shape,zoom", [(SMALL, 1.4), (SMALL, 1.125), (LARGE, 1.4), (LARGE, 1.125)])
def test_deformed_patch_matches_restatement(store, shape, zoom, grid):
    """Labels exact -- both sides round the same float32 coordinates; images (no gamma) within the bound of
    test_rotated_patch_matches_restatement, |got - ref| <= 2^-24 (|m| / s + 16 max(1, max |ref|)): coordinates and fractions are
    the same bits, so the float32 rounding is that of the subtraction, the scale and three lerps.  Lattices at the cap and (odd
    rows) at a quarter of it; every sample unrotated, at 17 and at 45 degrees.  The last row and column of the patch -- cell
    G - 1 at f = 1 -- are part of every comparison."""
    samples = _samples(shape, zoom)                    # the eight corners of case 0, its interior under all flips, cases 2 and 3
    rows = [(ci, c, crop, f, _sc(a), 1) for ci, c, crop, f in samples for a in ANGLES]
    # a quarter of the cap moves a coordinate by a fraction of a pixel, and not every such field carries a rounded coordinate
    # across a label boundary: each row takes the generator's first lattice whose RESTATED labels differ from the restated
    # undeformed ones, so that "the GPU's labels moved" below is a statement about the kernel
    px = dref.cap(shape[1:], grid)
    rng = np.random.default_rng(100 * grid + shape[1])
    lat, wants, redrawn = [], [], 0
    for j, (ci, c, crop, flips, sc, _) in enumerate(rows):
        im, lb = store["cases"][ci]
        still = dref.patch(im, lb, c, crop, shape, np.zeros((2, grid + 3, grid + 3), np.float32), grid, sc, flips)[1]
        for attempt in range(16):
            cand, info = dref.lattice(rng, px / 4 if j % 2 else px, grid), {}
            want = dref.patch(im, lb, c, crop, shape, cand, grid, sc, flips, info=info)
            if not np.array_equal(want[1], still):
                break
        assert not np.array_equal(want[1], still), (j, rows[j])
        redrawn += attempt
        lat.append(cand)
        wants.append(want + (info,))
    lat = np.stack(lat)
    assert redrawn <= len(rows) // 4                                                 # most first draws serve
    tab = _table(store, rows)
    got, lab = _run(store, tab, shape, lat, grid)
    lab1 = _run(store, tab, shape, lat, grid, lab_max=1)[1]
    undeformed = _run(store, _table(store, [r[:5] + (0,) for r in rows]), shape, lat, grid)[1]
    worst, outside, beyond = 0.0, 0, 0
    for j, (ci, c, crop, flips, sc, _) in enumerate(rows):
        want, want_lab, m, s, info = wants[j]
        np.testing.assert_array_equal(lab[j], want_lab, err_msg=str(rows[j]))
        np.testing.assert_array_equal(lab1[j], np.minimum(want_lab, 1), err_msg=str(rows[j]))
        assert s > 0 and info["invalid"] == 0
        bound = 2.0 ** -24 * (abs(m) / s + 16 * max(1.0, np.abs(want).max()))
        err = np.abs(got[j].astype(np.float64) - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (rows[j], err, bound)
        assert not np.array_equal(lab[j], undeformed[j]), (j, rows[j])                  # the deformation moved the labels
        outside += info["outside"]
        beyond += info["beyond"]
    print("lits_patch3d_warp {} zoom {} G {} PX {:.3f}: max error / bound = {:.3f}; taps outside the slice {}, beyond the crop box "
          "{}".format(shape, zoom, grid, px, worst, outside, beyond))
    assert outside > 0                                                               # the corner samples leave the slice
    box = ref.crop_box((6, 19, 23), samples[0][2], shape, ref.DEPTHS[0], (ref.H, ref.W))
    if box[3:] == (ref.H, ref.W):
        assert zoom == 1.4 and shape == LARGE                                        # the crop clamped to the slice: nothing beyond it
    else:
        assert beyond > 0                                                            # real tissue beyond the crop box
    assert {int(v) for v in np.unique(lab)} == {0, 1, 2}
    j = 3 * (len(samples) - 3)                                                       # the shallow case: zero slices stay zero
    assert np.all(got[j][5] == 0) and np.all(lab[j][5] == 0) and np.abs(got[j][4]).max() > 0


# ------------------------------------------------------------------------------------------------- 4. gamma
def test_gamma_on_deformed_patches_matches_restatement(store):
    """The bound of test_gamma_on_rotated_patches_matches_restatement: four times the measured deviation of powf from float64
    pow."""
    gammas = [0.7, 0.85, 1.0, 1.2, 1.5]
    worst, min_sd = 0.0, np.inf
    for (shape, zoom), grid in (((SMALL, 1.125), 3), ((LARGE, 1.4), 4)):
        samples = _samples(shape, zoom)
        rows = [s + (_sc(ANGLES[j % 3]), 1) for j, s in enumerate(samples)]
        g = [gammas[j % len(gammas)] for j in range(len(rows))]
        lat, _ = _lattices(len(rows), shape, grid, 40 + grid, quarter_every=2)
        tab = _table(store, rows, g)
        got, lab = _run(store, tab, shape, lat, grid, training=True)
        np.testing.assert_array_equal(lab, _run(store, tab, shape, lat, grid)[1])     # gamma leaves the labels alone
        for j, (ci, c, crop, flips, sc, _) in enumerate(rows):
            im, lb = store["cases"][ci]
            want = dref.patch(im, lb, c, crop, shape, lat[j], grid, sc, flips, gamma=g[j])[0]
            assert np.all(np.isfinite(got[j]))
            worst = max(worst, np.abs(got[j].astype(np.float64) - want).max())
            min_sd = min(min_sd, want.std())
    print("lits_patch3d_warp gamma: max |got - ref| = {:.3e}, smallest patch std = {:.3f}".format(worst, min_sd))
    bound = 4 * GAMMA_MAX_DEV_MEASURED
    assert bound < 1e-4 * min_sd
    assert worst <= bound


# ------------------------------------------------------------------------------------------------- 5. guide
@pytest.mark.parametrize("shape,grid", [(SMALL, 3), (LARGE, 4), (SMALL, 1)])
@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0)])
def test_deformed_guide_matches_restatement(store, shape, grid, stddev):
    """The bounds of test_rotated_guide_matches_restatement.  Euclidean: 8 * 2^-24 * max(1, largest distance) / normaliser over
    the corners the deformed grid visits.  Gaussian: four times the measured deviation of expf."""
    from boxsegliver_amd import ops
    samples, pts, cnt = _guide_inputs(shape)           # flips among them; a sample without fg, without bg, without any click
    idx = [i for i in range(len(samples)) for _ in ANGLES]
    rows = [samples[i] + (_sc(ANGLES[j % 3]), 1) for j, i in enumerate(idx)]
    tab = _table(store, rows)
    lat, _ = _lattices(len(rows), shape, grid, 60 + grid, quarter_every=2)
    warp = torch.from_numpy(lat).cuda()
    dp, dc = torch.from_numpy(pts[idx]).cuda(), torch.from_numpy(cnt[idx]).cuda()
    norm = cref.euclid_norm(shape[1])
    g2 = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 2, stddev, warp=warp, grid=grid)
    g1 = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 1, stddev, warp=warp, grid=grid)
    assert g2.shape == (len(rows),) + shape + (2,) and g1.shape == (len(rows),) + shape + (1,) and g2.dtype == torch.float32
    assert torch.equal((g2[..., 0] - g2[..., 1]).view(torch.int32), g1[..., 0].view(torch.int32))     # G = 1 is fg - bg, bit for bit
    again = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 2, stddev, warp=warp, grid=grid)
    assert torch.equal(g2.view(torch.int32), again.view(torch.int32))
    got = g2.cpu().numpy()
    worst = 0.0
    for j, (ci, c, crop, flips, sc, _) in enumerate(rows):
        i = idx[j]
        box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
        want, far = dref.sp_guide((shape[0],) + box[3:], shape[1:], pts[i], cnt[i], lat[j], grid, sc, flips, stddev, 2, norm)
        err = np.abs(got[j].astype(np.float64) - want).max()
        worst = max(worst, err)
        if stddev is None:
            tol = 8 * 2.0 ** -24 * max(1.0, far) / norm
            assert err <= tol, (j, err, tol)
        for kind in range(2):
            if cnt[i, kind] == 0:
                assert np.all(got[j][..., kind] == 0)                                 # a kind without clicks is exactly 0
            else:
                assert got[j][..., kind].max() > 0
    print("click_guide3d_warp {} G {} stddev {}: max |got - ref| = {:.3e}".format(shape, grid, stddev, worst))
    if stddev is not None:
        assert worst <= 4 * GAUSS_MAX_DEV_MEASURED


def test_click_lands_where_the_deformed_label_shows_the_object(store):
    """A single-voxel object: the simulator clicks on it in the UNDEFORMED crop, and the deformed guide peaks at the voxel
    where the deformed label shows the object, or within one voxel of it -- unrotated and rotated.  The crop is half the output,
    so every crop voxel stays the nearest one of some output voxel where the field compresses the patch."""
    from boxsegliver_amd import ops
    shape, crop, grid = SMALL, (8, 10), 3
    lb = torch.zeros_like(store["lb"])
    base = int(store["base"][3])
    mark = (4, 17, 29)                                                               # (slice of case 3, row, column)
    lb[base + mark[0], mark[1], mark[2]] = 2 * ref.LB_SCALE
    centre = (4, 19, 27)
    angles = (None, 17.0, None, 45.0, None, -33.0, None, 90.0)
    rows = [(3, centre, crop, FLIPS[j % 8], _sc(a), 1) for j, a in enumerate(angles)]
    tab = _table(store, rows)
    lat = np.stack([dref.lattice(np.random.default_rng(70 + j), dref.cap(shape[1:], grid) / 2, grid) for j in range(len(rows))])
    warp = torch.from_numpy(lat).cuda()
    clicks = np.zeros((len(rows), 12), np.uint32)
    clicks[:, 0], clicks[:, 2] = 1, 1                                                # one foreground click, no background click
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    pts, cnt = ops.lits3d_clicks(lb, tab, torch.from_numpy(clicks.view(np.int32)).cuda(), shape, status, 2)
    z1, y1, x1, _, _ = ref.crop_box(centre, crop, shape, ref.DEPTHS[3], (ref.H, ref.W))
    want = (mark[0] - z1, mark[1] - y1, mark[2] - x1)
    assert int(status.item()) == 0 and cnt.cpu().tolist() == [[1, 0]] * len(rows)
    assert pts[:, 0, 0].cpu().tolist() == [list(want)] * len(rows)                    # the deformation leaves the clicks alone
    labels = ops.lits_patch3d(store["im"], lb, tab, shape, False, warp=warp, grid=grid)[1].cpu().numpy()
    rot = ops.lits_patch3d(store["im"], lb, tab, shape, False, rotate=True)[1].cpu().numpy()
    moved = 0
    for stddev in ((1.0, 3.0, 3.0), None):
        g = ops.click_guide3d(tab, pts, cnt, shape, (ref.H, ref.W), 2, stddev, warp=warp, grid=grid).cpu().numpy()
        assert np.all(g[..., 1] == 0)
        for j in range(len(rows)):
            at = np.argwhere(labels[j] == 2)
            assert len(at) >= 1, j
            peak = np.unravel_index(np.argmax(g[j][..., 0]) if stddev else np.argmin(g[j][..., 0]), shape)
            assert np.abs(at - np.array(peak)).max(axis=1).min() <= 1, (j, at, peak)
            moved += int(not np.array_equal(labels[j], rot[j]))
    assert moved >= len(rows)                                                        # the field moved the object in most rows


# ------------------------------------------------------------------------------------------------- 6. bounds
def _hostile(shape, grid, zoom=1.4):
    """(rows, lattices): lattices of NaN, infinities, 1e30 and 2^20 -- whole and as single entries --, column 15 = -1 and 2^31 - 1,
    hostile (sin, cos) beside them, and ordinary rows of every kind around them."""
    samples = _samples(shape, zoom)
    rng = np.random.default_rng(90 + grid)
    px = dref.cap(shape[1:], grid)
    g = grid + 3

    def one(value, comp=None, at=None):
        lat = dref.lattice(rng, px, grid)
        if at is not None:
            lat[comp][at] = value
        elif comp is not None:
            lat[comp] = value
        else:
            lat[:] = value
        return lat
    big = 2.0 ** 20
    plan = [(one(np.nan), None, 1), (one(np.inf, 0, (0, 0)), None, -1), (one(-np.inf, 1), None, 2 ** 31 - 1),
            (one(1e30), None, 1), (one(big), None, -1), (one(-big, 0), rref.sincos(17.0), 1),
            (one(np.nan, 1, (0, 0)), (np.nan, 1.0), 2 ** 31 - 1), (one(big), (big, 0.0), 1), (one(0.0), (1e30, 0.5), -1),
            (one(np.inf), (0.0, -np.inf), 1), (one(1e30, 0, (g - 1, g - 1)), None, -1),
            (one(0.0), None, 2 ** 31 - 1), (one(0.0), None, -1)]
    rows = [samples[(3 * j) % len(samples)][:3] + ((j & 1, 0, (j >> 1) & 1), sc, flag) for j, (_, sc, flag) in enumerate(plan)]
    lats = [p[0] for p in plan]
    for j in range(0, len(samples), 2):
        rows.append(samples[j] + (rref.sincos(33.0) if j % 3 else None, (0, 1)[(j // 2) % 2]))
        lats.append(one(np.nan) if rows[-1][5] == 0 else dref.lattice(rng, px, grid))
    return rows, np.stack(lats), len(plan)


@pytest.mark.parametrize("training", [False, True])
def test_hostile_lattices_guard_bands_and_workspace(store, training):
    """Every output of the hostile rows is finite and is zero where the coordinate is invalid; nothing outside the outputs and
    the workspace is written; bad arguments are refused before anything is written; two calls give identical bits."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    shape, grid = LARGE, 4
    rows, lat, n_hostile = _hostile(shape, grid)
    n = len(rows)
    tab = _table(store, rows, [0.9] * n)
    warp = guardbuf.guarded_input(torch.from_numpy(lat).cuda().reshape(n, -1, 1))
    desc = ops.lits3d_desc(store["im"], n, shape, training)
    nbytes = int(lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(desc)))
    assert nbytes > 0 and nbytes % 16 == 0
    images = guardbuf.guarded((n,) + shape + (1,))
    labels = guardbuf.guarded((n,) + shape + (1,))                                   # int32 labels in a 4-byte guarded buffer
    ws = guardbuf.GuardedWorkspace(nbytes)
    head = (ctypes.byref(desc), _abi.ptr(store["im"]), _abi.ptr(store["lb"]), _abi.ptr(tab))
    tail = (ctypes.c_void_p(images.ptr()), ctypes.c_void_p(labels.ptr()), ctypes.c_void_p(ws.ptr()))
    wp = ctypes.c_void_p(warp.ptr())
    call = lib.unetk_lits_patch3d_warp
    assert call(*head, wp, grid, *tail, nbytes - 1, _abi.stream_ptr()) == -3          # UNETK_E_WORKSPACE, nothing launched
    for g, p in ((0, wp), (17, wp), (-1, wp), (grid, None), (grid, ctypes.c_void_p(warp.ptr() + 2))):
        assert call(*head, p, g, *tail, nbytes, _abi.stream_ptr()) == -1, g           # UNETK_E_BADARG
    torch.cuda.synchronize()
    assert images.changed_anywhere() == 0 and labels.changed_anywhere() == 0 and ws.guard_intact()
    assert call(*head, wp, grid, *tail, nbytes, _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert images.check_untouched() and images.unwritten() == 0
    assert labels.check_untouched() and labels.unwritten() == 0
    assert ws.guard_intact() and warp.changed_anywhere() == 0
    got = images.view[..., 0].cpu().numpy()
    lab = labels.view.view(torch.int32)[..., 0].cpu().numpy()
    assert np.all(np.isfinite(got)) and lab.min() >= 0 and lab.max() <= 2
    some_valid = all_invalid = 0
    for j, (ci, c, crop, flips, sc, flag) in enumerate(rows[:n_hostile]):
        box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
        ok = ref.flip(np.broadcast_to(dref.coords(shape[1:], box[3:], lat[j], grid, sc)[2], shape), flips)
        assert np.all(lab[j][~ok] == 0), (j, sc)
        if not training:                               # gamma shifts the zeros of a patch that is not all zeros
            assert np.all(got[j][~ok] == 0), (j, sc)
            im, lb = store["cases"][ci]
            want, want_lab, m, s = dref.patch(im, lb, c, crop, shape, lat[j], grid, sc, flips)
            np.testing.assert_array_equal(lab[j], want_lab)
            assert np.abs(got[j] - want).max() <= 2.0 ** -24 * (abs(m) / s + 16 * max(1.0, np.abs(want).max()))
        some_valid += int(ok.any() and not ok.all())
        all_invalid += int(not ok.any())
    assert some_valid >= 2 and all_invalid >= 2        # single hostile entries spoil their 4 x 4 support only
    # two calls give identical bits, through the wrapper too
    a = ops.lits_patch3d(store["im"], store["lb"], tab, shape, training, warp=torch.from_numpy(lat).cuda(), grid=grid)
    assert torch.equal(images.view.view(torch.int32), a[0].view(torch.int32))
    assert torch.equal(labels.view.view(torch.int32)[..., 0], a[1])
    # argument validation, as the _rot entry
    big = ops.lits3d_desc(store["im"], 1, (2048, 1024, 1024), training)
    assert call(ctypes.byref(big), *head[1:], wp, grid, *tail, nbytes, _abi.stream_ptr()) == -2           # UNETK_E_UNSUPPORTED
    assert call(head[0], None, *head[2:], wp, grid, *tail, nbytes, _abi.stream_ptr()) == -1
    assert call(*head, wp, grid, *tail[:2], ctypes.c_void_p(ws.ptr() + 8), nbytes, _abi.stream_ptr()) == -1


def test_hostile_lattices_guide_guard_bands(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    shape, grid = LARGE, 4
    samples, pts, cnt = _guide_inputs(shape)
    hostile, lat, n_hostile = _hostile(shape, grid)
    idx = [j % 4 for j in range(n_hostile)] + [0, 1, 2, 3, 4]
    rows = [samples[i][:3] + h[3:] for i, h in zip(idx[:n_hostile], hostile)] + \
           [samples[i] + (rref.sincos(33.0) if i % 2 else None, 1) for i in idx[n_hostile:]]
    lat = lat[:len(rows)].copy()
    lat[n_hostile:] = dref.lattice(np.random.default_rng(5), dref.cap(shape[1:], grid), grid, n=len(rows) - n_hostile)
    n = len(rows)
    tab = _table(store, rows)
    warp = torch.from_numpy(lat).cuda()
    dp, dc = torch.from_numpy(pts[idx]).cuda(), torch.from_numpy(cnt[idx]).cuda()
    for g, stddev in ((2, (1.0, 3.0, 3.0)), (1, None), (2, None)):
        desc = ops.lits3d_clicks_desc(store["lb"], n, shape, guide_channel=g, stddev=stddev, euclid_norm=cref.euclid_norm(shape[1]))
        out = guardbuf.guarded((n,) + shape + (g,))
        args = (ctypes.byref(desc), _abi.ptr(tab))
        rest = (_abi.ptr(dp), _abi.ptr(dc), ctypes.c_void_p(out.ptr()), _abi.stream_ptr())
        for wg, p in ((0, _abi.ptr(warp)), (17, _abi.ptr(warp)), (grid, None)):
            assert lib.unetk_click_guide3d_warp(*args, p, wg, *rest) == -1             # UNETK_E_BADARG
        torch.cuda.synchronize()
        assert out.changed_anywhere() == 0
        assert lib.unetk_click_guide3d_warp(*args, _abi.ptr(warp), grid, *rest) == 0
        torch.cuda.synchronize()
        assert out.check_untouched() and out.unwritten() == 0
        want = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), g, stddev, warp=warp, grid=grid)
        assert torch.equal(out.view.view(torch.int32), want.view(torch.int32))
        got = out.view.cpu().numpy()
        assert np.all(np.isfinite(got))
        for j, (ci, c, crop, flips, sc, flag) in enumerate(rows[:n_hostile]):
            box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
            ok = ref.flip(np.broadcast_to(dref.coords(shape[1:], box[3:], lat[j], grid, sc)[2], shape), flips)
            assert np.all(got[j][~ok] == 0), (g, stddev, j, sc)
            if g == 2 and stddev is None:
                want_j, far = dref.sp_guide((shape[0],) + box[3:], shape[1:], pts[idx[j]], cnt[idx[j]], lat[j], grid, sc, flips, None,
                                            2, cref.euclid_norm(shape[1]))
                assert np.abs(got[j] - want_j).max() <= 8 * 2.0 ** -24 * max(1.0, far) / cref.euclid_norm(shape[1]), (j, sc)


# ------------------------------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("extra", ["", "--random_rotate 20", "--use_spatial --local_enhance", "--random_rotate 20 --use_spatial"])
def test_liver_3d_trains_with_random_deform_from_the_command_line(tmp_path, extra):
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = ("liver_3d --mode train --tag cli3dd --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 2 --batches_per_epoch 2 --eval_num_batches_per_epoch 2 --eval_per_epoch --evaluator Volume "
            "--primary_metric Tumor/Dice --secondary_metric Liver/Dice --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --save_best --log_step 1").split() + extra.split()
    paths = ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    deform = ["--random_deform", "1.5", "--deform_grid", "3"]
    argv_on, argv_zero, argv_plain = argv + deform + paths, argv + ["--random_deform", "0", "--deform_grid", "3"] + paths, argv + paths

    def first(av, n):
        args, _, _ = entry.get_arguments(av)
        params = {"args": args, "lits_root": str(tmp_path)}
        gen = lits3d.input_fn("train", params)
        return [next(gen) for _ in range(n)], params
    (plain,), _ = first(argv_plain, 1)
    (zero,), _ = first(argv_zero, 1)
    assert sorted(plain[0]) == sorted(zero[0])
    for key in plain[0]:                                                             # --random_deform 0 is the run without the flag
        assert torch.equal(plain[0][key], zero[0][key]), key
    assert torch.equal(plain[1], zero[1])
    batches, params = first(argv_on, 3)
    for feats, labels in batches:
        assert feats["images"].shape == (2, 4, 32, 32, 1) and labels.shape == (2, 4, 32, 32)
        assert bool(torch.isfinite(feats["images"]).all()) and 0 <= int(labels.min()) and int(labels.max()) <= 2
        if "--use_spatial" in extra:
            assert feats["sp_guide"].shape == (2, 4, 32, 32, 2) and bool(torch.isfinite(feats["sp_guide"]).all())
            assert 0.0 <= float(feats["sp_guide"].min())
    assert not torch.equal(batches[0][0]["images"], plain[0]["images"])              # the first batch is deformed
    ev = list(lits3d.input_fn("eval_online", params))                                # evaluation never deforms; it reads the status
    plain_args, _, _ = entry.get_arguments(argv_plain)
    ev_plain = list(lits3d.input_fn("eval_online", {"args": plain_args, "lits_root": str(tmp_path)}))
    for (fa, la), (fb, lb) in zip(ev, ev_plain):
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(la, lb)
    assert int(params[("lits3d_status", True)].item()) == 0 and int(params[("lits3d_status", False)].item()) == 0
    # the command line
    assert entry.main(argv_on) == 0
    status = json.load(open(str(run / "checkpoint")))
    assert status["global_step"] == 2 and os.path.exists(str(run / status["model_checkpoint_path"]))
    losses = [float(v) for v in re.findall(r"loss = ([^,\s]+)", open(str(run / "logs" / "train_cli3dd")).read())]
    assert len(losses) >= 2 and all(np.isfinite(v) for v in losses)
