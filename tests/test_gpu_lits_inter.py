"""GPU: the click-guided LiTS batch kernels (`unetk_lits_inter_batch`, `unetk_lits_clicks`, `unetk_click_guide`;
csrc/lits_inter.hip) against the restatement of the reference's interactive pipeline (lits_inter_ref.py, which cites the
lines and uses scipy's binary_erosion literally), and `liver_inter` training the four click-guided nets from the command
line on a tiny dataset in the reference's on-disk format."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import guardbuf
import lits_inter_ref as ref
from click_shapes import rank_draw as _rank_draw

pytestmark = pytest.mark.gpu

H, W = 40, 48                                 # the slices of lits3d_ref.make_cases
SMALL_CLICKS = (1, 3, 5, 5)                   # margin, step, band, max_clicks on 40 x 48 slices
REF_CLICKS = (3, 10, 40, 5)                   # the reference's (gen_kernel :548-560)
BRIGHT = (17, 29)                             # the one bright pixel of the extra case's middle slice
# Gamma path: max |got - float64 restatement| over test_gamma_matches_restatement's samples, measured on an MI355X
# (ROCm 7 powf); asserted at four times that, the margin lits3d's GAMMA_MAX_DEV_MEASURED gets for another compiler's powf.
GAMMA_MAX_DEV_MEASURED = 1.624e-6


def _extra_case():
    """Three slices whose middle one is far brighter than its neighbours: z-scored together, channels 0 and 2 of a C = 3 sample
    centred on slice 1 are negative throughout (the channel mask zeroes them); one pixel of slice 1 outshines the rest."""
    rng = np.random.default_rng(23)
    im = np.stack([1000 + rng.integers(0, 10, (H, W)), 20000 + rng.integers(0, 100, (H, W)), 1000 + rng.integers(0, 10, (H, W))])
    im[1][BRIGHT] = 60000
    lab = np.zeros((3, H, W), np.uint8)
    lab[1, 10:30, 12:40] = 1
    return im.astype(np.uint16), lab


@pytest.fixture(scope="module")
def store():
    cases = ref.make_cases() + [_extra_case()]
    im, lb, base = ref.stack_store(cases)
    return dict(cases=cases, base=base, im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy(lb).cuda())


def _table(store, samples, gammas=None):
    """samples: (case, (cz, cy, cx), crop, (flip_lr, flip_ud))."""
    rows = [ref.table_row(store["base"][ci], store["cases"][ci][0].shape[0], c, crop, (f[0], f[1], 0),
                          1.0 if gammas is None else gammas[j]) for j, (ci, c, crop, f) in enumerate(samples)]
    return torch.from_numpy(np.stack(rows)).cuda()


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------- clicks
def _click_cases(params):
    """(case, centre, crop, obj_label, click_tab row, what the row is there for)."""
    last = 0xFFFFFFFF
    small = params == SMALL_CLICKS
    rows = [
        (0, (6, 20, 22), (32, 36), 1, [3, 2, 1, 0, 0, last, 7 << 28, 0, last, 0, 5 << 29, 0], "erosion"),          # liver: ranks 0, count - 1
        (0, (6, 20, 22), (32, 36), 1, [4, 4, 3, 0, 1 << 31, 3, 4, 5, 1 << 30, 0, 0, 0], "strategy3"),
        (0, (5, 20, 17), (32, 36), 2, [2, 3, 3, 0, 9, 9, 9, 9, 0, 0, 0, 0], "small+tie"),                           # one tumour pixel
        (1, (0, 20, 22), (30, 30), 1, [1, 2, 1, 0, 5, 5, 5, 5, 5, 5, 5, 5], "no object"),
        (1, (0, 20, 22), (30, 30), 1, [1, 0, 3, 0, 5, 5, 5, 5, 5, 5, 5, 5], "no object, n_bg = 0"),
        (0, (6, 20, 22), (6, 8), 1, [2, 3, 1, 0, 1 << 31, 1 << 30, 0, 0, 1, 2, 3, 4], "all object"),
        (0, (7, 20, 23), (32, 36), 2, [3, 1, 1, 0, _rank_draw(5, 12), 0, 0, 0, last, 0, 0, 0], "emptied"),          # the 5 x 6 blob
        (0, (0, 1, 1), (20, 24), 2, [1, 4, 3, 0, last, 0, 0, 0, 1 << 29, 0, 0, 0], "corner blob"),                   # 3 x 3 at the corner
        (3, (2, 17, 21), (44, 60), 2, [4, 4, 1, 0, 1, 2 << 30, 3 << 30, last, last, 0, 1 << 31, 1 << 30], "clamped crop"),
        (2, (2, 39, 0), (17, 23), 1, [2, 2, 3, 0, 6 << 28, 0, 0, 0, 9 << 28, 0, 0, 0], "odd crop at the border"),
    ]
    return rows if small else rows[:3] + rows[5:7] + rows[8:]


def _restated_clicks(store, rows, params):
    want_p, want_c, traces = [], [], []
    for ci, c, crop, obj_label, row, _ in rows:
        lab = store["cases"][ci][1]
        obj = ref.object_crop(lab, c[0], ref.crop_box(c[1:], crop, (H, W)), obj_label)
        tr = {}
        p, n = ref.clicks(obj, np.array(row, np.uint64), params, tr)
        tr["obj"] = obj
        want_p.append(p)
        want_c.append(n)
        traces.append(tr)
    return np.stack(want_p), np.stack(want_c), traces


def _run_clicks(store, rows, params):
    from boxsegliver_amd import ops
    out = []
    for obj_label in (1, 2):                                    # one launch per object label, rows kept in order
        idx = [j for j, r in enumerate(rows) if r[3] == obj_label]
        if not idx:
            continue
        tab = _table(store, [(rows[j][0], rows[j][1], rows[j][2], (j & 1, (j >> 1) & 1)) for j in idx])     # flips do not matter
        ctab = torch.from_numpy(np.array([rows[j][4] for j in idx], np.uint32).view(np.int32)).cuda()
        status = _status()
        a = ops.lits_clicks(store["lb"], tab, ctab, status, obj_label, params)
        b = ops.lits_clicks(store["lb"], tab, ctab, status, obj_label, params)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                                          # identical bits
        assert int(status.item()) == 0
        out.append((idx, a[0].cpu().numpy(), a[1].cpu().numpy()))
    pts = np.zeros((len(rows), 2, 4, 2), np.int32)
    cnt = np.zeros((len(rows), 2), np.int32)
    for idx, p, c in out:
        pts[idx], cnt[idx] = p, c
    return pts, cnt


def test_clicks_equal_the_restatement_small_parameters(store):
    rows = _click_cases(SMALL_CLICKS)
    want_p, want_c, tr = _restated_clicks(store, rows, SMALL_CLICKS)
    by = {r[5]: j for j, r in enumerate(rows)}
    # the inputs hold every situation -- asserted on the restatement alone, before the device is asked
    j = by["erosion"]
    assert not tr[j]["fg"]["small"] and want_c[j, 0] >= 2 and tr[j]["fg"]["ranks"][:2] == [0, tr[j]["fg"]["counts"][1] - 1]
    assert tr[j]["bg"]["band_cut"] and not tr[j]["bg"]["small"]                                       # the band leaves the crop
    assert tr[j]["bg"]["ranks"] == [tr[j]["bg"]["counts"][0] - 1, 0]
    j = by["small+tie"]
    assert tr[j]["fg"]["small"] and want_c[j, 0] == 1 and tr[j]["obj"].sum() == 1
    assert want_c[j, 1] == 3 and tr[j]["bg"]["ties"] >= 1                                             # strategy 3, a distance tie
    j = by["strategy3"]
    assert want_c[j, 1] >= 3 and want_c[j, 0] >= 3
    for j in (by["no object"], by["no object, n_bg = 0"]):
        assert tr[j]["obj"].max() == 0 and want_c[j, 0] == 0
    assert want_c[by["no object"], 1] == 1 and tuple(want_p[by["no object"], 1, 0]) == (14, 14)       # the crop's centre
    assert want_c[by["no object, n_bg = 0"]].tolist() == [0, 0]
    j = by["all object"]
    assert tr[j]["obj"].min() == 1 and want_c[j, 1] == 0 and want_c[j, 0] >= 1
    j = by["emptied"]
    assert tr[j]["fg"]["emptied"] and want_c[j, 0] == 1 and rows[j][4][0] == 3                        # one click left nothing
    assert tr[by["clamped crop"]]["obj"].shape == (H, W) and tr[by["odd crop at the border"]]["obj"].shape == (17, 23)
    pts, cnt = _run_clicks(store, rows, SMALL_CLICKS)
    for j, r in enumerate(rows):
        np.testing.assert_array_equal(cnt[j], want_c[j], err_msg=r[5])
        np.testing.assert_array_equal(pts[j], want_p[j], err_msg=r[5])


def test_clicks_equal_the_restatement_reference_parameters(store):
    rows = _click_cases(REF_CLICKS)
    want_p, want_c, tr = _restated_clicks(store, rows, REF_CLICKS)
    assert not tr[0]["fg"]["small"] and tr[2]["fg"]["small"] and want_c[:, 1].max() >= 3
    pts, cnt = _run_clicks(store, rows, REF_CLICKS)
    for j, r in enumerate(rows):
        np.testing.assert_array_equal(cnt[j], want_c[j], err_msg=r[5])
        np.testing.assert_array_equal(pts[j], want_p[j], err_msg=r[5])


def test_clicks_guard_bands_and_bad_rows(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    rows = [r for r in _click_cases(SMALL_CLICKS) if r[3] == 1]
    n = len(rows)
    tab = _table(store, [(r[0], r[1], r[2], (0, 0)) for r in rows])
    ctab = torch.from_numpy(np.array([r[4] for r in rows], np.uint32).view(np.int32)).cuda()
    desc = ops.lits_inter_desc(store["lb"], n, (1, 1, 1), obj_label=1, clicks=SMALL_CLICKS)
    nbytes = int(lib.unetk_lits_clicks_ws_bytes(ctypes.byref(desc)))
    assert nbytes >= n * 3 * H * W and nbytes % 16 == 0
    pts, cnt, ws = guardbuf.guarded((n, 2, 4, 2)), guardbuf.guarded((n, 2)), guardbuf.GuardedWorkspace(nbytes)
    status = _status()
    args = (ctypes.byref(desc), _abi.ptr(store["lb"]), _abi.ptr(tab), _abi.ptr(ctab), ctypes.c_void_p(pts.ptr()),
            ctypes.c_void_p(cnt.ptr()), _abi.ptr(status), ctypes.c_void_p(ws.ptr()))
    assert lib.unetk_lits_clicks(*args, nbytes - 1, _abi.stream_ptr()) == -3                          # nothing launched
    torch.cuda.synchronize()
    assert pts.changed_anywhere() == 0 and cnt.changed_anywhere() == 0
    assert lib.unetk_lits_clicks(*args, nbytes, _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert pts.check_untouched() and pts.unwritten() == 0 and cnt.check_untouched() and cnt.unwritten() == 0
    assert ws.guard_intact() and int(status.item()) == 0
    want = ops.lits_clicks(store["lb"], tab, ctab, status, 1, SMALL_CLICKS)
    assert torch.equal(pts.view.view(torch.int32), want[0]) and torch.equal(cnt.view.view(torch.int32), want[1])
    # bad rows: a centre slice outside the case or the store has no object (bit 1); draws out of range are clamped (bit 2)
    bad = torch.from_numpy(np.stack([ref.table_row(store["base"][0], 12, (15, 20, 22), (30, 30)),
                                     ref.table_row(10 ** 6, 9, (4, 20, 22), (30, 30)),
                                     ref.table_row(store["base"][0], 12, (-3, 2 ** 30, -2 ** 30), (2 ** 30, -5))])).cuda()
    draws = torch.from_numpy(np.array([[1, 1, 1, 0] + [7] * 8] * 3, np.uint32).view(np.int32)).cuda()
    status = _status()
    p, c = ops.lits_clicks(store["lb"], bad, draws, status, 1, SMALL_CLICKS)
    assert int(status.item()) == 2
    np.testing.assert_array_equal(c.cpu().numpy(), [[0, 1]] * 3)
    np.testing.assert_array_equal(p[:, 1, 0].cpu().numpy(), [[14, 14], [14, 14], [19, 0]])            # the crops' centres
    row = rows[0]
    for col, val in ((0, 0), (0, 5), (1, 5), (2, 2)):
        t = np.array([row[4]], np.uint32)
        t[0, col] = val
        status = _status()
        got = ops.lits_clicks(store["lb"], tab[:1].contiguous(), torch.from_numpy(t.view(np.int32)).cuda(), status, 1, SMALL_CLICKS)
        t[0, col] = {(0, 0): 1, (0, 5): 4, (1, 5): 4, (2, 2): 1}[(col, val)]                           # the clamped value
        obj = ref.object_crop(store["cases"][row[0]][1], row[1][0], ref.crop_box(row[1][1:], row[2], (H, W)), 1)
        wp, wc = ref.clicks(obj, t[0].astype(np.uint64), SMALL_CLICKS)
        assert int(status.item()) == 4, (col, val)
        np.testing.assert_array_equal(got[0][0].cpu().numpy(), wp)
        np.testing.assert_array_equal(got[1][0].cpu().numpy(), wc)


# ------------------------------------------------------------------------------------------------- images and labels
def _image_samples(c, out_hw):
    """crop = output; a crop clamped by the slice; cz at 0 and depth - 1 (padding slices); all four flips; an odd crop."""
    d0 = 12
    out = [(0, (6, 19, 23), out_hw, (i & 1, i >> 1)) for i in range(4)]
    out += [(0, (6, 19, 23), (44, 60), (1, 0)), (0, (0, 1, 1), (33, 37), (0, 1)), (0, (d0 - 1, 38, 46), (27, 41), (1, 1)),
            (3, (2, 17, 21), (36, 40), (0, 0)), (4, (1, 20, 24), (30, 34), (0, 1))]
    return out


def _run_images(store, samples, shape, training=False, obj_label=1, gammas=None, noise=0.0, seed=0):
    from boxsegliver_amd import ops
    status = _status()
    images, labels = ops.lits_inter_batch(store["im"], store["lb"], _table(store, samples, gammas), shape, training, status,
                                          obj_label, noise, seed)
    assert images.shape == (len(samples), shape[1], shape[2], shape[0]) and images.dtype == torch.float32
    assert labels.shape == (len(samples), shape[1], shape[2]) and labels.dtype == torch.int32
    assert int(status.item()) == 0
    return images.cpu().numpy(), labels.cpu().numpy()


@pytest.mark.parametrize("shape", [(3, 24, 28), (1, 24, 28), (3, 72, 68)])
def test_images_and_labels_match_restatement(store, shape):
    """Labels exact; images (no gamma) within the float32 rounding of the subtraction, the scale and three lerps, the bound of
    test_gpu_lits3d.test_patch_matches_restatement: |got - ref| <= 2^-24 (|m| / s + 16 max(1, max |ref|))."""
    samples = _image_samples(shape[0], shape[1:])
    got, lab = _run_images(store, samples, shape)
    lab2 = _run_images(store, samples, shape, obj_label=2)[1]
    worst = 0.0
    for j, (ci, c, crop, flips) in enumerate(samples):
        im, lb = store["cases"][ci]
        want, want_lab, m, s = ref.sample(im, lb, c, crop, shape, flips)
        np.testing.assert_array_equal(lab[j], want_lab, err_msg=str(samples[j]))
        np.testing.assert_array_equal(lab2[j], ref.sample(im, lb, c, crop, shape, flips, obj_label=2)[1], err_msg=str(samples[j]))
        assert s > 0
        bound = 2.0 ** -24 * (abs(m) / s + 16 * max(1.0, np.abs(want).max()))
        err = np.abs(got[j].astype(np.float64) - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (samples[j], err, bound)
    print("lits_inter_batch {}: max error / bound = {:.3f}".format(shape, worst))
    assert set(np.unique(lab).tolist()) == {0, 1} and lab2.max() == 1 and (lab2 <= lab).all()
    if shape[0] == 3:                                           # the padding slices: zeros before the first / after the last slice
        assert np.all(got[5][..., 0] == 0) and np.abs(got[5][..., 1]).max() > 0
        assert np.all(got[6][..., 2] == 0) and np.abs(got[6][..., 1]).max() > 0


def test_gamma_matches_restatement(store):
    """augment_gamma(retain_stats=True) over the whole [H, W, C] image against the float64 restatement.  powf differs from
    float64 pow by an amount that is measured, not derived: GAMMA_MAX_DEV_MEASURED, asserted at four times that."""
    shape = (3, 24, 28)
    samples = _image_samples(3, shape[1:])
    gammas = [0.7, 0.85, 1.0, 1.2, 1.5, 0.75, 1.35, 0.9, 1.1]
    got, lab = _run_images(store, samples, shape, training=True, gammas=gammas)
    np.testing.assert_array_equal(lab, _run_images(store, samples, shape)[1])
    worst, min_sd = 0.0, np.inf
    for j, (ci, c, crop, flips) in enumerate(samples):
        im, lb = store["cases"][ci]
        want = ref.sample(im, lb, c, crop, shape, flips, gamma=gammas[j])[0]
        assert np.all(np.isfinite(got[j]))
        worst = max(worst, np.abs(got[j].astype(np.float64) - want).max())
        min_sd = min(min_sd, want.std())
    print("lits_inter_batch gamma: max |got - ref| = {:.3e}, smallest image std = {:.3f}".format(worst, min_sd))
    bound = 4 * GAMMA_MAX_DEV_MEASURED
    assert bound < 1e-4 * min_sd
    assert worst <= bound


def test_noise_is_the_restated_generator_and_the_channel_mask_is_exact(store):
    shape = (3, 24, 28)
    samples = _image_samples(3, shape[1:])
    gammas = [0.8 + 0.05 * j for j in range(len(samples))]
    plain = _run_images(store, samples, shape, training=True, gammas=gammas)[0]
    for seed, scale in ((12345, 0.1), (0xFEDCBA98, 0.03)):
        want, keep = ref.noise_and_mask(plain, seed, scale)
        assert keep[-1].tolist() == [0, 1, 0] and keep[:4].min() == 1                 # the extra case: two channels below zero
        got = _run_images(store, samples, shape, training=True, gammas=gammas, noise=scale, seed=seed)[0]
        np.testing.assert_array_equal(got, want)
        assert np.all(got[-1][..., 0] == 0) and np.all(got[-1][..., 2] == 0)
    a = _run_images(store, samples, shape, training=True, gammas=gammas, noise=0.1, seed=7)[0]
    b = _run_images(store, samples, shape, training=True, gammas=gammas, noise=0.1, seed=7)[0]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))                          # two calls, identical bits
    # evaluation batches take neither gamma nor noise
    ev = _run_images(store, samples, shape, training=False, gammas=gammas, noise=0.1, seed=7)[0]
    assert np.array_equal(ev.view(np.int32), _run_images(store, samples, shape)[0].view(np.int32))


def test_images_guard_bands_and_status(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    shape = (3, 24, 28)
    samples = _image_samples(3, shape[1:])
    n = len(samples)
    tab = _table(store, samples, [0.9] * n)
    desc = ops.lits_inter_desc(store["im"], n, shape, True, 1, noise_scale=0.1, seed=3)
    nbytes = int(lib.unetk_lits_inter_batch_ws_bytes(ctypes.byref(desc)))
    assert nbytes > 0 and nbytes % 16 == 0
    images, labels, ws = guardbuf.guarded((n, 24, 28, 3)), guardbuf.guarded((n, 24, 28, 1)), guardbuf.GuardedWorkspace(nbytes)
    status = _status()
    args = (ctypes.byref(desc), _abi.ptr(store["im"]), _abi.ptr(store["lb"]), _abi.ptr(tab), ctypes.c_void_p(images.ptr()),
            ctypes.c_void_p(labels.ptr()), _abi.ptr(status), ctypes.c_void_p(ws.ptr()))
    assert lib.unetk_lits_inter_batch(*args, nbytes - 1, _abi.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert images.changed_anywhere() == 0 and labels.changed_anywhere() == 0
    assert lib.unetk_lits_inter_batch(*args, nbytes, _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert images.check_untouched() and images.unwritten() == 0 and labels.check_untouched() and labels.unwritten() == 0
    assert ws.guard_intact() and int(status.item()) == 0
    want = ops.lits_inter_batch(store["im"], store["lb"], tab, shape, True, status, 1, 0.1, 3)
    assert torch.equal(images.view.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(labels.view.view(torch.int32)[..., 0], want[1])
    # a centre slice outside the case: zeros, label 0, bit 1 of the status word
    bad = torch.from_numpy(np.stack([ref.table_row(store["base"][0], 12, (20, 19, 23), (24, 28))])).cuda()
    im, lb = ops.lits_inter_batch(store["im"], store["lb"], bad, shape, False, status, 1)
    assert int(status.item()) == 2 and not im.any() and not lb.any()
    with pytest.raises(_abi.UnetkError, match="device tensors"):
        ops.lits_inter_batch(store["im"].cpu(), store["lb"].cpu(), tab.cpu(), shape, False, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_abi.UnetkError, match="unsupported shape"):
        ops.lits_inter_batch(store["im"], store["lb"], tab, (2, 24, 28), False, status)


# ------------------------------------------------------------------------------------------------- guide
def _guide_inputs(store):
    samples = [(0, (6, 19, 23), (24, 28), (0, 0)), (0, (6, 19, 23), (30, 33), (1, 0)), (0, (0, 1, 1), (33, 37), (0, 1)),
               (3, (2, 17, 21), (44, 60), (1, 1)), (1, (3, 30, 30), (17, 23), (1, 0))]
    pts = np.full((len(samples), 2, 4, 2), -1, np.int32)
    cnt = np.zeros((len(samples), 2), np.int32)
    pts[0, 0, :2], cnt[0] = [(3, 4), (20, 27)], (2, 0)                                # no background click
    pts[1, 0, :1], pts[1, 1, :4], cnt[1] = [(15, 16)], [(0, 0), (29, 32), (0, 32), (29, 0)], (1, 4)
    pts[2, 1, :3], cnt[2] = [(5, 5), (6, 30), (32, 36)], (0, 3)                       # no foreground click
    pts[3, 0, :3], pts[3, 1, :1], cnt[3] = [(20, 24), (21, 24), (39, 47)], [(0, 47)], (3, 1)
    return samples, pts, cnt                                                          # sample 4: no click at all


@pytest.mark.parametrize("stddev", [None, 5.0, 2.5])
def test_guide_matches_restatement(store, stddev):
    from boxsegliver_amd import ops
    samples, pts, cnt = _guide_inputs(store)
    tab = _table(store, samples)
    out_hw = (24, 28)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda()
    g2 = ops.click_guide(tab, dp, dc, out_hw, (H, W), 2, stddev)
    g1 = ops.click_guide(tab, dp, dc, out_hw, (H, W), 1, stddev)
    assert g2.shape == (len(samples), 24, 28, 2) and g1.shape == (len(samples), 24, 28, 1) and g2.dtype == torch.float32
    assert torch.equal((g2[..., 0] - g2[..., 1]).view(torch.int32), g1[..., 0].view(torch.int32))     # G = 1 is fg - bg, bit for bit
    assert torch.equal(g2.view(torch.int32), ops.click_guide(tab, dp, dc, out_hw, (H, W), 2, stddev).view(torch.int32))
    got = g2.cpu().numpy()
    for j, (ci, c, crop, flips) in enumerate(samples):
        box = ref.crop_box(c[1:], crop, (H, W))
        want, far = ref.sp_guide(box[2:], out_hw, pts[j], cnt[j], flips, stddev)
        tol = 2e-6 if stddev is not None else 8 * 2.0 ** -24 * max(1.0, far)
        err = np.abs(got[j].astype(np.float64) - want).max()
        assert err <= tol, (j, err, tol)
        for kind in range(2):
            if cnt[j, kind] == 0:
                assert np.all(got[j][..., kind] == 0)                                 # a kind without clicks is exactly 0
            else:
                assert got[j][..., kind].max() > 0


def test_guide_flips_line_up_with_the_image(store):
    """A click on the bright pixel stays on it under every flip: crop = output, so crop pixels are output pixels."""
    from boxsegliver_amd import ops
    crop = (24, 28)
    centre = (1, BRIGHT[0] + 2, BRIGHT[1] - 3)
    samples = [(4, centre, crop, (i & 1, i >> 1)) for i in range(4)]
    y1, x1, _, _ = ref.crop_box(centre[1:], crop, (H, W))
    click = (BRIGHT[0] - y1, BRIGHT[1] - x1)
    assert 0 < click[0] < crop[0] - 1 and 0 < click[1] < crop[1] - 1
    pts = np.full((4, 2, 4, 2), -1, np.int32)
    pts[:, 0, 0] = click
    cnt = np.tile(np.array([[1, 0]], np.int32), (4, 1))
    tab = _table(store, samples)
    images = _run_images(store, samples, (1,) + crop)[0][..., 0]
    seen = set()
    for stddev in (4.0, None):
        g = ops.click_guide(tab, torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda(), crop, (H, W), 2, stddev).cpu().numpy()[..., 0]
        for j in range(4):
            at = np.unravel_index(np.argmax(images[j]), crop)
            guide_at = np.unravel_index(np.argmax(g[j]) if stddev else np.argmin(g[j]), crop)
            assert at == guide_at, (j, at, guide_at)
            seen.add(at)
    assert len(seen) == 4                                                            # the four flips are four places


# ------------------------------------------------------------------------------------------------- end to end
def _argv(tmp_path, run, model, extra):
    argv = ("liver_inter --mode train --tag inter --model {} --classes Tumor --test_fold 1 --im_height 32 --im_width 32 "
            "--im_channel 3 --random_flip 3 --noise_scale 0.05 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--batches_per_epoch 2 --eval_num_batches_per_epoch 2 --eval_per_epoch --evaluator Volume "
            "--primary_metric Tumor/Dice --loss_weight_type numerical --loss_numeric_w 1 1 --learning_rate 0.001 --save_best "
            "--log_step 1 --use_spatial").format(model).split()
    return argv + extra + ["--lits_root", str(tmp_path), "--model_dir", str(run)]


def test_liver_inter_trains_unetinter_from_the_command_line(tmp_path):
    from boxsegliver_amd.data import lits_inter
    from boxsegliver_amd.entry import main_g
    from boxsegliver_amd.entry import main as entry
    ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = _argv(tmp_path, run, "UNetInter", "--num_of_steps 4 --local_enhance --stddev 5.".split())
    args, _, _ = entry.get_arguments(argv, guided=True)
    params = {"args": args, "lits_root": str(tmp_path)}
    gen = lits_inter.input_fn("train", params)
    forced_seen = 0
    for _ in range(6):
        feats, labels = next(gen)
        assert feats["images"].shape == (2, 32, 32, 3) and feats["images"].dtype == torch.float32 and feats["images"].is_cuda
        assert feats["sp_guide"].shape == (2, 32, 32, 2) and feats["sp_guide"].dtype == torch.float32 and feats["sp_guide"].is_cuda
        assert labels.shape == (2, 32, 32) and labels.dtype == torch.int32 and labels.is_cuda
        assert bool(torch.isfinite(feats["images"]).all()) and bool(torch.isfinite(feats["sp_guide"]).all())
        assert 0 <= float(feats["sp_guide"].min()) and float(feats["sp_guide"].max()) <= 1          # the Gaussian guide
        assert 0 <= int(labels.min()) and int(labels.max()) <= 1
        assert feats["names"].tolist() == [0, 1]                                      # forced: the tumour case; then the other
        forced_seen += int((labels[0] == 1).any())
        assert not bool((labels[1] == 1).any())                                       # case 1 has no tumour
        assert float(feats["sp_guide"][0, ..., 0].max()) > 0.5 or not bool((labels[0] == 1).any())   # a foreground click
    assert forced_seen >= 3                                                           # centred on a tumour voxel (a flip keeps it)
    ev = [list(lits_inter.input_fn("eval_online", params)) for _ in range(2)]
    assert len(ev[0]) == 2
    for (fa, la), (fb, lb) in zip(*ev):                                               # every evaluation scores the same batches
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(fa["sp_guide"], fb["sp_guide"]) and torch.equal(la, lb)
        assert sorted(fa["names"].tolist()) == [2, 3]
    assert int(params[("lits_inter_status", True)].item()) == 0 and int(params[("lits_inter_status", False)].item()) == 0
    params[("lits_inter_status", True)].fill_(4)
    with pytest.raises(RuntimeError, match="training batches.*click draws"):
        next(lits_inter.input_fn("eval_online", params))
    params[("lits_inter_status", True)].zero_()
    # the command line
    assert entry.main(argv) == 0
    status = json.load(open(str(run / "checkpoint")))
    assert status["global_step"] == 4 and os.path.exists(str(run / status["model_checkpoint_path"]))
    losses = [float(v) for v in re.findall(r"loss = ([^,\s]+)", open(str(run / "logs" / "train_inter")).read())]
    assert len(losses) >= 4 and all(np.isfinite(v) for v in losses)
    assert "Tumor/Dice" in json.load(open(str(run / "best_result")))
    argv_eval = list(argv)
    argv_eval[argv_eval.index("--mode") + 1] = "eval"
    for main in (entry.main, main_g.main):
        with pytest.raises(NotImplementedError, match="offline evaluator"):
            main(argv_eval)


@pytest.mark.parametrize("model,extra", [("SmallUNet", "--local_enhance --stddev 5."), ("InterUNet", "--local_enhance --stddev 5."),
                                         ("LGNet", "--guide_channel 1")])
def test_liver_inter_steps_the_other_click_guided_nets(tmp_path, model, extra):
    from boxsegliver_amd.entry import main as entry
    ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = _argv(tmp_path, run, model, ["--num_of_steps", "1"] + extra.split())
    argv = [a for a in argv if a != "--eval_per_epoch"]
    assert entry.main(argv) == 0
    status = json.load(open(str(run / "checkpoint")))
    assert status["global_step"] == 1
    losses = [float(v) for v in re.findall(r"loss = ([^,\s]+)", open(str(run / "logs" / "train_inter")).read())]
    assert len(losses) >= 1 and all(np.isfinite(v) for v in losses)
