"""GPU: in-plane rotated LiTS 3-D patches and their click guides (`unetk_lits_patch3d_rot`, `unetk_click_guide3d_rot`;
csrc/lits3d.hip, csrc/lits3d_clicks.hip) against np.rot90 of the plain entries at the quarter turns, against the
plain entries bit for bit on rows that are not rotated, against the restatement (lits3d_rotate_ref.py) at general angles, on
hostile table contents inside guard bands, and `liver_3d --random_rotate` training UNet3D from the command line."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import guardbuf
import lits3d_clicks_ref as cref
import lits3d_ref as ref
import lits3d_rotate_ref as rref
from test_gpu_lits3d import GAMMA_MAX_DEV_MEASURED, _samples
from test_gpu_lits3d_clicks import GAUSS_MAX_DEV_MEASURED, _guide_inputs

pytestmark = pytest.mark.gpu

SMALL, LARGE, SQUARE = (6, 16, 20), (6, 32, 40), (6, 16, 16)      # test_gpu_lits3d.py's shapes and one square one
ANGLES = (17.0, -33.0, 45.0, 180.0)
QUARTERS = (((0.0, 1.0), 0), ((1.0, 0.0), 3), ((0.0, -1.0), 2), ((-1.0, 0.0), 1))      # (sin, cos) -> k of np.rot90
FLIPS = [(i & 1, (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]
# the last one is finite and large: 2^20 times the offset from the centre crosses 2^24 inside the patch, so the row mixes valid
# coordinates (far outside the slice) with invalid ones
HOSTILE = ((np.nan, np.nan), (np.nan, 1.0), (np.inf, 0.0), (0.0, -np.inf), (1e30, 0.5), (0.5, -1e30), (-0.0, -0.0), (-0.0, 0.0),
           (2.0 ** 20, 0.0))


@pytest.fixture(scope="module")
def store():
    cases = ref.make_cases()
    im, lb, base = ref.stack_store(cases)
    return dict(cases=cases, base=base, im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy(lb).cuda())


def _table(store, rows, gammas=None):
    """rows: (case, centre, crop, flips, (sin, cos) or None)."""
    out = [rref.table_row(store["base"][ci], ref.DEPTHS[ci], c, crop, flips, 1.0 if gammas is None else gammas[j], sc)
           for j, (ci, c, crop, flips, sc) in enumerate(rows)]
    return torch.from_numpy(np.stack(out)).cuda()


def _run(store, tab, shape, training=False, lab_max=2, rotate=True):
    from boxsegliver_amd import ops
    images, labels = ops.lits_patch3d(store["im"], store["lb"], tab, shape, training, lab_max, rotate=rotate)
    assert images.shape == (tab.shape[0],) + tuple(shape) + (1,) and images.dtype == torch.float32
    assert labels.shape == (tab.shape[0],) + tuple(shape) and labels.dtype == torch.int32
    return images[..., 0].cpu().numpy(), labels.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------- 1. quarter turns
def test_quarter_turns_equal_rot90_of_the_plain_entry(store):
    """Square crop at zoom 1: the coordinates are exact integers, so image and label are np.rot90 of the plain entry's, bit for
    bit, under all eight flips; the explicit identity (0, 1) is the plain entry's output."""
    crop = SQUARE[1:]
    places = [(0, (6, 19, 23)), (0, (0, 0, 0)), (0, (11, 39, 47)), (2, (2, 17, 21)), (3, (5, 20, 40))]
    plain = _run(store, _table(store, [(ci, c, crop, (0, 0, 0), None) for ci, c in places]), SQUARE, rotate=False)
    rows = [(ci, c, crop, f, sc) for ci, c in places for f in FLIPS for sc, _ in QUARTERS]
    tab = _table(store, rows)
    got, lab = _run(store, tab, SQUARE)
    flipped = _run(store, tab, SQUARE, rotate=False)                                   # the plain entry ignores the columns
    j = 0
    for p in range(len(places)):
        for f in FLIPS:
            for sc, k in QUARTERS:
                want = ref.flip(np.rot90(plain[0][p], k, axes=(1, 2)), f)
                want_lab = ref.flip(np.rot90(plain[1][p], k, axes=(1, 2)), f)
                assert np.array_equal(_bits(got[j]), _bits(want)), (places[p], f, sc)
                np.testing.assert_array_equal(lab[j], want_lab, err_msg=str((places[p], f, sc)))
                if k == 0:
                    assert np.array_equal(_bits(got[j]), _bits(flipped[0][j])) and np.array_equal(lab[j], flipped[1][j])
                j += 1
    assert np.abs(plain[0]).max() > 0 and {int(v) for v in np.unique(plain[1])} == {0, 1, 2}
    assert not np.array_equal(got[1], got[0])                                          # a quarter turn moves the patch


# ------------------------------------------------------------------------------------------------- 2. unrotated rows
@pytest.mark.parametrize("training", [False, True])
def test_rows_that_are_not_rotated_are_the_plain_entry_bit_for_bit(store, training):
    samples = _samples(LARGE, 1.4) + _samples(LARGE, 1.125)[:5]
    rows = [(ci, c, crop, f, None if j % 2 == 0 else rref.sincos(ANGLES[(j // 2) % 4])) for j, (ci, c, crop, f) in enumerate(samples)]
    gammas = [0.7 + 0.04 * j for j in range(len(rows))]
    tab = _table(store, rows, gammas)
    got = _run(store, tab, LARGE, training)
    plain = _run(store, tab, LARGE, training, rotate=False)
    for j, row in enumerate(rows):
        same = np.array_equal(_bits(got[0][j]), _bits(plain[0][j])) and np.array_equal(got[1][j], plain[1][j])
        assert same == (row[4] is None), (j, row)
    # an all-zero table through the _rot entry is the plain entry's batch
    zero = _table(store, [r[:4] + (None,) for r in rows], gammas)
    a, b = _run(store, zero, LARGE, training), _run(store, zero, LARGE, training, rotate=False)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0)])
def test_guide_rows_that_are_not_rotated_are_the_plain_entry_bit_for_bit(store, stddev):
    from boxsegliver_amd import ops
    samples, pts, cnt = _guide_inputs(LARGE)
    keep = [0, 1, 2, 3, 4, 0, 1, 3]
    rows = [samples[i] + (None if j % 2 == 0 else rref.sincos(ANGLES[j % 4]),) for j, i in enumerate(keep)]
    tab = _table(store, rows)
    dp, dc = torch.from_numpy(pts[keep]).cuda(), torch.from_numpy(cnt[keep]).cuda()
    for g in (1, 2):
        got = ops.click_guide3d(tab, dp, dc, LARGE, (ref.H, ref.W), g, stddev, rotate=True).cpu().numpy()
        plain = ops.click_guide3d(tab, dp, dc, LARGE, (ref.H, ref.W), g, stddev).cpu().numpy()
        for j, i in enumerate(keep):
            same = np.array_equal(_bits(got[j]), _bits(plain[j]))
            assert same == (rows[j][4] is None or cnt[i].sum() == 0), (g, j)           # sample 4 has no click: all zeros


# ------------------------------------------------------------------------------------------------- 3. general angles
@pytest.mark.parametrize("shape,zoom", [(SMALL, 1.4), (SMALL, 1.125), (LARGE, 1.4)])
def test_rotated_patch_matches_restatement(store, shape, zoom):
    """Labels exact -- both sides round the same float32 coordinates; images (no gamma) within the bound of
    test_patch_matches_restatement, |got - ref| <= 2^-24 (|m| / s + 16 max(1, max |ref|)): the coordinates and fractions are the
    same bits, so the float32 rounding is that of the subtraction, the scale and three lerps, as there."""
    samples = _samples(shape, zoom)                    # the eight corners of case 0, its interior under all flips, cases 2 and 3
    rows = [(ci, c, crop, f, rref.sincos(a)) for ci, c, crop, f in samples for a in ANGLES]
    tab = _table(store, rows)
    got, lab = _run(store, tab, shape)
    lab1 = _run(store, tab, shape, lab_max=1)[1]
    worst, outside, beyond = 0.0, 0, 0
    for j, (ci, c, crop, flips, sc) in enumerate(rows):
        im, lb = store["cases"][ci]
        info = {}
        want, want_lab, m, s = rref.patch(im, lb, c, crop, shape, sc, flips, info=info)
        np.testing.assert_array_equal(lab[j], want_lab, err_msg=str(rows[j]))
        np.testing.assert_array_equal(lab1[j], np.minimum(want_lab, 1), err_msg=str(rows[j]))
        assert s > 0 and info["invalid"] == 0
        bound = 2.0 ** -24 * (abs(m) / s + 16 * max(1.0, np.abs(want).max()))
        err = np.abs(got[j].astype(np.float64) - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (rows[j], err, bound)
        outside += info["outside"]
        beyond += info["beyond"]
    print("lits_patch3d_rot {} zoom {}: max error / bound = {:.3f}; taps outside the slice {}, beyond the crop box {}".format(
        shape, zoom, worst, outside, beyond))
    assert outside > 0                                                               # the corner samples leave the slice
    box = ref.crop_box((6, 19, 23), samples[0][2], shape, ref.DEPTHS[0], (ref.H, ref.W))
    if zoom == 1.4 and shape == LARGE:
        assert box[3:] == (ref.H, ref.W)                                             # the crop clamped to the slice: nothing beyond it
    else:
        assert beyond > 0                                                            # real tissue in the corners of a turned patch
    assert {int(v) for v in np.unique(lab)} == {0, 1, 2}
    # the shallow case: slices beyond its depth stay zeros with label 0
    j = 4 * (len(samples) - 3)
    assert np.all(got[j][5] == 0) and np.all(lab[j][5] == 0) and np.abs(got[j][4]).max() > 0


# ------------------------------------------------------------------------------------------------- 4. gamma
def test_gamma_on_rotated_patches_matches_restatement(store):
    """The bound of test_gamma_matches_restatement: four times its measured deviation of powf from float64 pow."""
    gammas = [0.7, 0.85, 1.0, 1.2, 1.5]
    worst, min_sd = 0.0, np.inf
    for shape, zoom in ((SMALL, 1.125), (LARGE, 1.4)):
        samples = _samples(shape, zoom)
        rows = [s + (rref.sincos(ANGLES[j % 4]),) for j, s in enumerate(samples)]
        g = [gammas[j % len(gammas)] for j in range(len(rows))]
        tab = _table(store, rows, g)
        got, lab = _run(store, tab, shape, training=True)
        np.testing.assert_array_equal(lab, _run(store, tab, shape)[1])                # gamma leaves the labels alone
        for j, (ci, c, crop, flips, sc) in enumerate(rows):
            im, lb = store["cases"][ci]
            want = rref.patch(im, lb, c, crop, shape, sc, flips, gamma=g[j])[0]
            assert np.all(np.isfinite(got[j]))
            worst = max(worst, np.abs(got[j].astype(np.float64) - want).max())
            min_sd = min(min_sd, want.std())
    print("lits_patch3d_rot gamma: max |got - ref| = {:.3e}, smallest patch std = {:.3f}".format(worst, min_sd))
    bound = 4 * GAMMA_MAX_DEV_MEASURED
    assert bound < 1e-4 * min_sd
    assert worst <= bound


# ------------------------------------------------------------------------------------------------- 5. guide
@pytest.mark.parametrize("shape", [SMALL, LARGE])
@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0)])
def test_rotated_guide_matches_restatement(store, shape, stddev):
    """The bounds of test_guide_matches_restatement.  Euclidean: 8 * 2^-24 * max(1, largest distance) / normaliser, the largest
    distance taken over the corners the rotated grid visits (they leave the crop box).  Gaussian: four times the measured
    deviation of expf."""
    from boxsegliver_amd import ops
    samples, pts, cnt = _guide_inputs(shape)           # flips among them; a sample without fg, without bg, without any click
    idx = [i for i in range(len(samples)) for _ in ANGLES]
    rows = [samples[i] + (rref.sincos(ANGLES[j % 4]),) for j, i in enumerate(idx)]
    tab = _table(store, rows)
    dp, dc = torch.from_numpy(pts[idx]).cuda(), torch.from_numpy(cnt[idx]).cuda()
    norm = cref.euclid_norm(shape[1])
    g2 = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 2, stddev, rotate=True)
    g1 = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 1, stddev, rotate=True)
    assert g2.shape == (len(rows),) + shape + (2,) and g1.shape == (len(rows),) + shape + (1,) and g2.dtype == torch.float32
    assert torch.equal((g2[..., 0] - g2[..., 1]).view(torch.int32), g1[..., 0].view(torch.int32))     # G = 1 is fg - bg, bit for bit
    again = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 2, stddev, rotate=True)
    assert torch.equal(g2.view(torch.int32), again.view(torch.int32))
    got = g2.cpu().numpy()
    worst = 0.0
    for j, (ci, c, crop, flips, sc) in enumerate(rows):
        i = idx[j]
        box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
        want, far = rref.sp_guide((shape[0],) + box[3:], shape[1:], pts[i], cnt[i], sc, flips, stddev, 2, norm)
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
    print("click_guide3d_rot {} stddev {}: max |got - ref| = {:.3e}".format(shape, stddev, worst))
    if stddev is not None:
        assert worst <= 4 * GAUSS_MAX_DEV_MEASURED


def test_click_lands_where_the_rotated_label_shows_the_object(store):
    """A single-voxel object: the simulator clicks on it ("small": the mask's mean) in the UNROTATED crop, and the rotated guide
    peaks at the voxel where the rotated label shows the object, or within one voxel of it.  The crop is smaller than the
    output, so every crop voxel is the nearest one of some output voxel under any angle."""
    from boxsegliver_amd import ops
    shape, crop = SMALL, (12, 15)
    lb = torch.zeros_like(store["lb"])
    base = int(store["base"][3])
    mark = (4, 17, 29)                                                               # (slice of case 3, row, column)
    lb[base + mark[0], mark[1], mark[2]] = 2 * ref.LB_SCALE
    centre = (4, 20, 25)
    rows = [(3, centre, crop, FLIPS[j % 8], rref.sincos(a)) for j, a in enumerate(ANGLES + (90.0, -90.0, 60.0, -120.0))]
    tab = _table(store, rows)
    clicks = np.zeros((len(rows), 12), np.uint32)
    clicks[:, 0], clicks[:, 2] = 1, 1                                                # one foreground click, no background click
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    pts, cnt = ops.lits3d_clicks(lb, tab, torch.from_numpy(clicks.view(np.int32)).cuda(), shape, status, 2)
    z1, y1, x1, _, _ = ref.crop_box(centre, crop, shape, ref.DEPTHS[3], (ref.H, ref.W))
    want = (mark[0] - z1, mark[1] - y1, mark[2] - x1)
    assert int(status.item()) == 0 and cnt.cpu().tolist() == [[1, 0]] * len(rows)
    assert pts[:, 0, 0].cpu().tolist() == [list(want)] * len(rows)                    # the rotation leaves the clicks alone
    labels = ops.lits_patch3d(store["im"], lb, tab, shape, False, rotate=True)[1].cpu().numpy()
    plain = ops.lits_patch3d(store["im"], lb, tab, shape, False)[1].cpu().numpy()
    seen = set()
    for stddev in ((1.0, 3.0, 3.0), None):
        g = ops.click_guide3d(tab, pts, cnt, shape, (ref.H, ref.W), 2, stddev, rotate=True).cpu().numpy()
        assert np.all(g[..., 1] == 0)
        for j in range(len(rows)):
            at = np.argwhere(labels[j] == 2)
            assert len(at) >= 1, j
            peak = np.unravel_index(np.argmax(g[j][..., 0]) if stddev else np.argmin(g[j][..., 0]), shape)
            assert np.abs(at - np.array(peak)).max(axis=1).min() <= 1, (j, at, peak)
            seen.add(tuple(at[0]))
            assert not np.array_equal(labels[j], plain[j])                            # the turn moved the object
    assert len(seen) >= 4                                                            # angles and flips put it in different places


# ------------------------------------------------------------------------------------------------- 6, 7. bounds
def _hostile_rows(shape, zoom):
    samples = _samples(shape, zoom)
    rows = [samples[(3 * j) % len(samples)][:3] + ((0, 0, 0), sc) for j, sc in enumerate(HOSTILE)]
    rows += [samples[j] + (rref.sincos(ANGLES[j % 4]) if j % 3 else None,) for j in range(0, len(samples), 2)]
    return rows


@pytest.mark.parametrize("training", [False, True])
def test_hostile_rows_guard_bands_and_workspace(store, training):
    """sin / cos bits of NaN, infinities, 1e30 and -0.0: every output of those rows is finite and is zero where the coordinate
    is invalid; nothing outside the outputs and the workspace is written; a short workspace is refused before anything is
    written; two calls give identical bits."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    shape = LARGE
    rows = _hostile_rows(shape, 1.4)
    n = len(rows)
    tab = _table(store, rows, [0.9] * n)
    desc = ops.lits3d_desc(store["im"], n, shape, training)
    nbytes = int(lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(desc)))
    assert nbytes > 0 and nbytes % 16 == 0
    images = guardbuf.guarded((n,) + shape + (1,))
    labels = guardbuf.guarded((n,) + shape + (1,))                                   # int32 labels in a 4-byte guarded buffer
    ws = guardbuf.GuardedWorkspace(nbytes)
    args = (ctypes.byref(desc), _abi.ptr(store["im"]), _abi.ptr(store["lb"]), _abi.ptr(tab), ctypes.c_void_p(images.ptr()),
            ctypes.c_void_p(labels.ptr()), ctypes.c_void_p(ws.ptr()))
    assert lib.unetk_lits_patch3d_rot(*args, nbytes - 1, _abi.stream_ptr()) == -3     # UNETK_E_WORKSPACE, nothing launched
    torch.cuda.synchronize()
    assert images.changed_anywhere() == 0 and labels.changed_anywhere() == 0 and ws.guard_intact()
    assert lib.unetk_lits_patch3d_rot(*args, nbytes, _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert images.check_untouched() and images.unwritten() == 0
    assert labels.check_untouched() and labels.unwritten() == 0
    assert ws.guard_intact()
    got = images.view[..., 0].cpu().numpy()
    lab = labels.view.view(torch.int32)[..., 0].cpu().numpy()
    assert np.all(np.isfinite(got)) and lab.min() >= 0 and lab.max() <= 2
    some_valid = 0
    for j, (ci, c, crop, flips, sc) in enumerate(rows[:len(HOSTILE)]):
        box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
        ok = rref.coords(shape[1:], box[3:], sc)[2]
        assert np.all(lab[j][:, ~ok] == 0), (j, sc)
        if not training:                               # gamma shifts the zeros of a patch that is not all zeros
            assert np.all(got[j][:, ~ok] == 0), (j, sc)
            im, lb = store["cases"][ci]
            want, want_lab, m, s = rref.patch(im, lb, c, crop, shape, sc, flips)
            np.testing.assert_array_equal(lab[j], want_lab)
            assert np.abs(got[j] - want).max() <= 2.0 ** -24 * (abs(m) / s + 16 * max(1.0, np.abs(want).max()))
        some_valid += int(ok.any() and not ok.all())
    assert some_valid >= 1                             # the 2^20 row: both sides of the 2^24 rule in one patch
    # two calls give identical bits, through the wrapper too
    a = ops.lits_patch3d(store["im"], store["lb"], tab, shape, training, rotate=True)
    assert torch.equal(images.view.view(torch.int32), a[0].view(torch.int32))
    assert torch.equal(labels.view.view(torch.int32)[..., 0], a[1])
    # argument validation, as the plain entry
    big = ops.lits3d_desc(store["im"], 1, (2048, 1024, 1024), training)
    assert lib.unetk_lits_patch3d_rot(ctypes.byref(big), *args[1:], nbytes, _abi.stream_ptr()) == -2      # UNETK_E_UNSUPPORTED
    assert lib.unetk_lits_patch3d_rot(ctypes.byref(desc), None, *args[2:], nbytes, _abi.stream_ptr()) == -1
    assert lib.unetk_lits_patch3d_rot(*args[:6], ctypes.c_void_p(ws.ptr() + 8), nbytes, _abi.stream_ptr()) == -1


def test_hostile_rows_guide_guard_bands(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    shape = LARGE
    samples, pts, cnt = _guide_inputs(shape)
    idx = [j % 4 for j in range(len(HOSTILE))] + [0, 1, 2, 3, 4]
    rows = [samples[i][:3] + ((0, 0, 0), sc) for i, sc in zip(idx, HOSTILE)] + [samples[i] + (rref.sincos(33.0),) for i in idx[len(HOSTILE):]]
    n = len(rows)
    tab = _table(store, rows)
    dp, dc = torch.from_numpy(pts[idx]).cuda(), torch.from_numpy(cnt[idx]).cuda()
    for g, stddev in ((2, (1.0, 3.0, 3.0)), (1, None), (2, None)):
        desc = ops.lits3d_clicks_desc(store["lb"], n, shape, guide_channel=g, stddev=stddev, euclid_norm=cref.euclid_norm(shape[1]))
        out = guardbuf.guarded((n,) + shape + (g,))
        assert lib.unetk_click_guide3d_rot(ctypes.byref(desc), _abi.ptr(tab), _abi.ptr(dp), _abi.ptr(dc), ctypes.c_void_p(out.ptr()),
                                           _abi.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert out.check_untouched() and out.unwritten() == 0
        want = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), g, stddev, rotate=True)
        assert torch.equal(out.view.view(torch.int32), want.view(torch.int32))
        got = out.view.cpu().numpy()
        assert np.all(np.isfinite(got))
        for j, (ci, c, crop, flips, sc) in enumerate(rows[:len(HOSTILE)]):
            box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
            ok = rref.coords(shape[1:], box[3:], sc)[2]
            assert np.all(got[j][:, ~ok] == 0), (g, stddev, j, sc)
            if g == 2 and stddev is None:
                want_j, far = rref.sp_guide((shape[0],) + box[3:], shape[1:], pts[idx[j]], cnt[idx[j]], sc, flips, None, 2,
                                            cref.euclid_norm(shape[1]))
                assert np.abs(got[j] - want_j).max() <= 8 * 2.0 ** -24 * max(1.0, far) / cref.euclid_norm(shape[1]), (j, sc)


# ------------------------------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("extra", ["", "--use_spatial --local_enhance"])
def test_liver_3d_trains_with_random_rotate_from_the_command_line(tmp_path, extra):
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = ("liver_3d --mode train --tag cli3dr --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 4 --batches_per_epoch 2 --eval_num_batches_per_epoch 2 --eval_per_epoch --evaluator Volume "
            "--primary_metric Tumor/Dice --secondary_metric Liver/Dice --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --save_best --log_step 1").split() + extra.split()
    paths = ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    argv_rot, argv_zero, argv_plain = argv + ["--random_rotate", "20"] + paths, argv + ["--random_rotate", "0"] + paths, argv + paths

    def first(av, n):
        args, _, _ = entry.get_arguments(av)
        params = {"args": args, "lits_root": str(tmp_path)}
        gen = lits3d.input_fn("train", params)
        return [next(gen) for _ in range(n)], params
    (plain,), _ = first(argv_plain, 1)
    (zero,), _ = first(argv_zero, 1)
    assert sorted(plain[0]) == sorted(zero[0])
    for key in plain[0]:                                                             # --random_rotate 0 is the run without the flag
        assert torch.equal(plain[0][key], zero[0][key]), key
    assert torch.equal(plain[1], zero[1])
    batches, params = first(argv_rot, 4)
    for feats, labels in batches:
        assert feats["images"].shape == (2, 4, 32, 32, 1) and labels.shape == (2, 4, 32, 32)
        assert bool(torch.isfinite(feats["images"]).all()) and 0 <= int(labels.min()) and int(labels.max()) <= 2
        if extra:
            assert feats["sp_guide"].shape == (2, 4, 32, 32, 2) and bool(torch.isfinite(feats["sp_guide"]).all())
            assert 0.0 <= float(feats["sp_guide"].min()) and float(feats["sp_guide"].max()) <= 1.0
    assert not torch.equal(batches[0][0]["images"], plain[0]["images"])              # the first batch is turned
    ev = list(lits3d.input_fn("eval_online", params))                                # evaluation never rotates; it reads the status
    plain_args, _, _ = entry.get_arguments(argv_plain)
    ev_plain = list(lits3d.input_fn("eval_online", {"args": plain_args, "lits_root": str(tmp_path)}))
    for (fa, la), (fb, lb) in zip(ev, ev_plain):
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(la, lb)
    assert int(params[("lits3d_status", True)].item()) == 0 and int(params[("lits3d_status", False)].item()) == 0
    # the command line
    assert entry.main(argv_rot) == 0
    status = json.load(open(str(run / "checkpoint")))
    assert status["global_step"] == 4 and os.path.exists(str(run / status["model_checkpoint_path"]))
    losses = [float(v) for v in re.findall(r"loss = ([^,\s]+)", open(str(run / "logs" / "train_cli3dr")).read())]
    assert len(losses) >= 4 and all(np.isfinite(v) for v in losses)
