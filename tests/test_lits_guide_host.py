"""CPU: the spatial guide of the guided LiTS pipeline (input_pipeline_g.py:382-412 render, :527-599 sampler policy).

`render_numpy` restates what the reference does per sample -- create_spatial_guide_2d at crop resolution, resize_bilinear
(align_corners) with lits_batch_kernel's crop clamp and flips, g / 2 + 0.5, exactly 0.5 without objects -- and is pinned here
on the reference's own numpy twin of the renderer (tests/golden/ref_sp_guide.npz, make_guide_fixtures.py).
tests/test_gpu_lits_guide.py holds `unetk_lits_spatial_guide` against it.  The sampler policy (`TrainSampler.guide_objects`)
is checked through its invariants."""
import argparse
import os

import numpy as np
import pytest

from boxsegliver_amd.data import lits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sp_guide.npz")
F32 = np.float32


def render_numpy(tab, obj_ptr, obj, out_hw, channels, src_hw, min_std=1.0):
    """f32 [N, H, W, 1]: per sample the guide rendered over the whole (clamped) crop, then resized and flipped."""
    tab, obj_ptr, obj = np.asarray(tab), np.asarray(obj_ptr), np.asarray(obj, F32).reshape(-1, 4)
    n, c = tab.shape[0], channels
    h, w = out_hw
    src_h, src_w = src_hw
    out = np.empty((n, h, w, 1), F32)
    for j in range(n):
        k0, k1 = int(obj_ptr[j]), int(obj_ptr[j + 1])
        if k1 <= k0:
            out[j] = 0.5
            continue
        off_y, off_x = min(max(int(tab[j, c + 1]), 0), src_h - 1), min(max(int(tab[j, c + 2]), 0), src_w - 1)
        ch, cw = min(max(int(tab[j, c + 3]), 1), src_h - off_y), min(max(int(tab[j, c + 4]), 1), src_w - off_x)
        o = obj[k0:k1]
        s = np.maximum(o[:, 2:], F32(min_std))
        ty = (np.arange(ch, dtype=F32)[None, :] - o[:, 0:1]) ** 2 / (F32(2) * s[:, 0:1] * s[:, 0:1])    # [K, ch]
        tx = (np.arange(cw, dtype=F32)[None, :] - o[:, 1:2]) ** 2 / (F32(2) * s[:, 1:2] * s[:, 1:2])    # [K, cw]
        g = np.exp(-(ty[:, :, None] + tx[:, None, :])).max(axis=0).astype(F32)                      # create_spatial_guide_2d

        def taps(size, crop, flip):
            o_ = np.arange(size)
            src = (size - 1 - o_) if flip else o_
            scale = F32(crop - 1) / F32(size - 1) if size > 1 else F32(0)
            p = src.astype(F32) * scale
            i0 = np.floor(p).astype(np.int64)
            return i0, np.minimum(i0 + 1, crop - 1), (p - i0.astype(F32)).astype(F32)

        y0, y1, ly = taps(h, ch, bool(tab[j, c + 6]))
        x0, x1, lx = taps(w, cw, bool(tab[j, c + 5]))
        tl, tr, bl, br = g[y0][:, x0], g[y0][:, x1], g[y1][:, x0], g[y1][:, x1]
        top, bot = tl + (tr - tl) * lx[None, :], bl + (br - bl) * lx[None, :]
        out[j, ..., 0] = (top + (bot - top) * ly[:, None]) / F32(2) + F32(0.5)
    return out


def test_restatement_reproduces_the_reference_renderer():
    """crop == output size: the resize is an identity, so the guide is g / 2 + 0.5 of create_gaussian_distribution_v2."""
    z = np.load(GOLDEN)
    assert len(z["shapes"]) >= 6
    for i, (h, w, k) in enumerate(z["shapes"].tolist()):
        obj = np.concatenate([z["case{}_centers".format(i)], z["case{}_stddevs".format(i)]], axis=1)
        tab = np.array([[0, 0, 0, 0, h, w, 0, 0]], np.int32)
        got = render_numpy(tab, [0, k], obj, (h, w), 1, (h, w))
        want = z["case{}_guide".format(i)] / F32(2) + F32(0.5)
        np.testing.assert_allclose(got[0, ..., 0], want, rtol=0, atol=2e-6, err_msg="case {}".format(i))


def test_restatement_flips_and_empty_samples():
    z = np.load(GOLDEN)
    h, w, k = z["shapes"][1].tolist()
    obj = np.concatenate([z["case1_centers"], z["case1_stddevs"]], axis=1)
    tab = np.array([[0, 0, 0, 0, h, w, f_lr, f_ud] for f_lr, f_ud in ((0, 0), (1, 0), (0, 1), (1, 1))] + [[0] * 8], np.int32)
    ptr = [0, k, 2 * k, 3 * k, 4 * k, 4 * k]
    got = render_numpy(tab, ptr, np.concatenate([obj] * 4), (h, w), 1, (h, w))
    np.testing.assert_array_equal(got[1], got[0][:, ::-1])
    np.testing.assert_array_equal(got[2], got[0][::-1])
    np.testing.assert_array_equal(got[3], got[0][::-1, ::-1])
    assert np.all(got[4] == F32(0.5))


# ------------------------------------------------------------------------------------------------- sampler policy
def _case(pid, depth=12, size=96):
    """A parsed case: tumour slices 4, 5, 7 with 1, 3 and 2 tumours (one near a border, one with a zero stddev)."""
    return {"PID": pid, "size": [depth, size, size], "bbox": [2, 20, 24, depth - 2, 70, 72],
            "tumor_slices_index": [4, 5, 7],
            "slices": [[[30, 34, 38, 40]], [[31, 33, 39, 41], [50, 52, 55, 58], [2, 2, 6, 6]], [[60, 60, 70, 70], [40, 20, 44, 26]]],
            "centers": [[[34.0, 37.0]], [[35.0, 37.0], [52.5, 55.0], [3.5, 4.0]], [[65.0, 65.0], [42.0, 23.0]]],
            "stddevs": [[[2.0, 2.0]], [[2.5, 1.5], [1.0, 0.0], [0.5, 0.5]], [[3.0, 3.0], [1.5, 2.0]]]}


CFG = argparse.Namespace(im_height=48, im_width=48, im_channel=3)


def _sampler(bs=16, seed=5, **kw):
    g = dict(spatial_random=1.0, inner_random=False, center_ratio=0.2, stddev_ratio=0.4, min_std=2.0)
    g.update(kw)
    cases = [_case(i) for i in range(3)]
    return cases, lits.TrainSampler(cases, bs, CFG, liver_percent=0.66, tumor_percent=0.5, random_scale=(1.0, 1.4),
                                    random_window_level=True, random_flip=3, seed=seed, guide=lits.GuidePolicy(**g))


def _tumours(case, z):
    if z not in case["tumor_slices_index"]:
        return np.zeros((0, 2), F32), np.zeros((0, 2), F32)
    i = case["tumor_slices_index"].index(z)
    return np.array(case["centers"][i], F32), np.array(case["stddevs"][i], F32)


def _in_box(c, box):
    off_y, off_x, ch, cw = box
    return (off_y <= c[:, 0]) & (c[:, 0] < off_y + ch) & (off_x <= c[:, 1]) & (c[:, 1] < off_x + cw)


def test_objects_are_the_in_box_tumours_perturbed_within_bounds():
    cases, smp = _sampler(center_ratio=0.2, stddev_ratio=0.4, min_std=2.0)
    seen = 0
    for _ in range(30):
        b = smp.draw()
        ptr, obj = smp.guide_objects(b)
        assert ptr.dtype == np.int32 and ptr.shape == (17,) and ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
        assert obj.dtype == np.float32 and obj.shape == (ptr[-1], 4)
        for j in range(16):
            c, s = _tumours(cases[int(b["case"][j])], int(b["z"][j]))
            inside = _in_box(c, b["box"][j])
            o = obj[ptr[j]:ptr[j + 1]]
            assert len(o) == int(inside.sum())                                    # spatial_random 1, no inner random: all in-box
            c, s = c[inside].astype(np.float64), s[inside].astype(np.float64)
            rel = c - b["box"][j][:2]
            assert np.all(np.abs(o[:, :2] - rel) <= 0.2 * s + 1e-4)               # |c' - (c - off)| <= r_c s
            lo = np.maximum(s / 1.4, 2.0)
            assert np.all(o[:, 2:] >= lo - 1e-5) and np.all(o[:, 2:] <= np.maximum(s * 1.4, 2.0) + 1e-5)
            assert np.all(o[:, 2:] >= 2.0)                                        # the sampler's min_std floor
            seen += len(o)
    assert seen > 50


def test_zero_ratios_keep_the_moments():
    cases, smp = _sampler(center_ratio=0.0, stddev_ratio=0.0, min_std=0.5)
    for _ in range(10):
        b = smp.draw()
        ptr, obj = smp.guide_objects(b)
        for j in range(16):
            c, s = _tumours(cases[int(b["case"][j])], int(b["z"][j]))
            inside = _in_box(c, b["box"][j])
            o = obj[ptr[j]:ptr[j + 1]]
            np.testing.assert_array_equal(o[:, :2], (c[inside].astype(np.float64) - b["box"][j][:2]).astype(F32))
            np.testing.assert_array_equal(o[:, 2:], np.maximum(s[inside], F32(0.5)))


def test_inner_random_subsets_are_non_empty_and_in_box():
    cases, smp = _sampler(inner_random=True, center_ratio=0.0, stddev_ratio=0.0)
    sizes, empty_in_box = set(), 0
    for _ in range(60):
        b = smp.draw()
        ptr, obj = smp.guide_objects(b)
        for j in range(16):
            c, _ = _tumours(cases[int(b["case"][j])], int(b["z"][j]))
            inside = _in_box(c, b["box"][j])
            o = obj[ptr[j]:ptr[j + 1]]
            if not inside.any():
                assert len(o) == 0                                                 # the reference raises here; no guide
                empty_in_box += len(c) > 0
                continue
            assert 1 <= len(o) <= int(inside.sum())
            rel = (c[inside].astype(np.float64) - b["box"][j][:2]).astype(F32)
            assert all(any(np.array_equal(p, q) for q in rel) for p in o[:, :2])  # drawn from the in-box set, no repeats
            assert len({tuple(p) for p in o[:, :2].tolist()}) == len(o)
            sizes.add((int(inside.sum()), len(o)))
    assert (2, 1) in sizes and (2, 2) in sizes                                     # both subset sizes of a 2-tumour box occur
    assert empty_in_box > 0                                                        # tumour slices whose tumours all fell outside


def test_spatial_random_zero_gives_no_objects_and_coin_rate():
    _, smp = _sampler(spatial_random=0.0)
    for _ in range(5):
        ptr, obj = smp.guide_objects(smp.draw())
        assert np.all(ptr == 0) and obj.shape == (0, 4)
    _, half = _sampler(spatial_random=0.5, bs=64)
    _, full = _sampler(spatial_random=1.0, bs=64)
    n_half = sum(int(half.guide_objects(half.draw())[0][-1]) for _ in range(40))
    n_full = sum(int(full.guide_objects(full.draw())[0][-1]) for _ in range(40))
    assert 0.35 * n_full < n_half < 0.65 * n_full


def test_guide_draws_leave_the_batch_stream_alone():
    """The guide has a generator of its own: the same seed draws the same batches with and without it."""
    cases, guided = _sampler(seed=9)
    plain = lits.TrainSampler(cases, 16, CFG, liver_percent=0.66, tumor_percent=0.5, random_scale=(1.0, 1.4),
                              random_window_level=True, random_flip=3, seed=9)
    offs = {c["PID"]: 100 * c["PID"] for c in cases}
    for _ in range(5):
        b = guided.draw()
        guided.guide_objects(b)
        t1, c1, p1 = guided.table(offs, b)
        t2, c2, p2 = plain.table(offs)
        np.testing.assert_array_equal(t1, t2)
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(p1, p2)


def test_slice_lookup_and_csr_gather():
    cases = [_case(0), _case(1, depth=9)]
    m = lits.ObjectMoments(cases)
    assert m.centers.shape == (12, 2) and m.stddevs.shape == (12, 2) and m.box_ptr.tolist() == [0, 1, 4, 6, 7, 10, 12]
    ind = m.slice_index([0, 0, 0, 1, 1, 1, 0], [4, 5, 6, 4, 7, -100, 7])
    assert ind.tolist() == [0, 1, -1, 3, 5, -1, 2]
    ptr, c, s = m.gather(ind)
    assert ptr.tolist() == [0, 1, 4, 4, 5, 7, 7, 9]
    np.testing.assert_array_equal(c[1:4], np.array(cases[0]["centers"][1], F32))
    np.testing.assert_array_equal(s[7:9], np.array(cases[0]["stddevs"][2], F32))
    empty = lits.ObjectMoments([dict(_case(0), tumor_slices_index=[], slices=[], centers=[], stddevs=[])])
    assert empty.slice_index([0, 0], [4, 5]).tolist() == [-1, -1]
    ptr, c, s = empty.gather(np.array([-1, -1]))
    assert ptr.tolist() == [0, 0, 0] and c.shape == (0, 2)


def test_moments_must_match_the_boxes():
    bad = _case(0)
    bad["centers"] = bad["centers"][:2] + [[[65.0, 65.0]]]
    with pytest.raises(ValueError):
        lits.ObjectMoments([bad])
