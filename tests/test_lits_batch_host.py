"""CPU: every row of the 2-D LiTS batch kernel's case table (lits_batch_cases.py) reaches what it is listed for, shown from the
references alone; the two references agree; the image bound is honest and sharp.  test_gpu_lits_batch_edges.py then holds
`unetk_lits_batch` to the same table on the device."""
import numpy as np
import pytest

import lits_batch_cases as lc
from lits_batch_cases import F32, GROUPS, STORES

GROUP_C = [(g.name, c) for g in GROUPS for c in lc.CHANNELS]


def _valid(idx, n):
    return 0 <= idx < n


@pytest.mark.parametrize("name,channels", GROUP_C)
def test_every_group_mixes_flips_and_special_slices(name, channels):
    g, st = lc.GROUP[name], STORES[lc.GROUP[name].store]
    rows = lc.rows_of(name, channels)
    assert {(r.flip_lr, r.flip_ud) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {r.box for r in rows} == set(g.boxes)
    assert any(-1 in r.chans for r in rows) and any(r.seg == -1 for r in rows)
    assert any(st.n in r.chans for r in rows)
    assert any(lc.INT32_MAX in r.chans for r in rows) and any(r.seg == lc.INT32_MAX for r in rows)
    for r in rows:
        assert lc.clamp_box(r.box, st.hw) == r.box                 # inside the slice: the clamp is the identity here
        assert len(r.chans) == channels and r.clip[1] > r.clip[0]
    tab, clip = lc.table(rows)
    assert tab.dtype == np.int32 and tab.shape == (len(rows), channels + 7) and clip.shape == (len(rows), 2)


def test_stores_are_what_the_rows_assume():
    for name, st in STORES.items():
        im, lb = lc.store(name)
        assert im.shape == (st.n,) + st.hw and im.dtype == np.uint16 and lb.shape == im.shape and lb.dtype == np.uint8
        assert im.min() < st.ends[0] and im.max() > st.ends[1]                          # a part of the pixels clips
        contrast = np.abs(np.diff(im.astype(np.int64), axis=2)).min()
        assert contrast > 0.9 * (st.ends[1] - st.ends[0])                                # high contrast everywhere
    lb = lc.store("small")[1]
    assert set(np.unique(lb[lc.EVERY_VALUE_SLICE]).tolist()) == set(range(256))
    cls = lc.store("big")[1][0].astype(np.int64) // lc.LB_SCALE
    for dy, dx in [(0, 1), (1, 0), (1, 1), (1, -1)]:                                     # every one-pixel shift changes the class
        a = cls[max(dy, 0):cls.shape[0] + min(dy, 0), max(dx, 0):cls.shape[1] + min(dx, 0)]
        b = cls[max(-dy, 0):cls.shape[0] + min(-dy, 0), max(-dx, 0):cls.shape[1] + min(-dx, 0)]
        assert np.all(a != b), (dy, dx)


# ------------------------------------------------------------------------------------------------- what each row is listed for
def _axis_pairs():
    """Every (crop, output) pair of one axis that a group row uses."""
    pairs = set()
    for g in GROUPS:
        for b in g.boxes:
            pairs.add((b[2], g.out_hw[0]))
            pairs.add((b[3], g.out_hw[1]))
    return sorted(pairs)


def _exact(crop, out):
    """(floor, twice the fractional part as an exact fraction numerator, denominator) of the exact coordinates."""
    k = np.arange(out, dtype=np.int64)
    den = max(out - 1, 1)
    num = k * (crop - 1) if out > 1 else k * 0
    return num // den, num % den, den


def test_tie_counts_match_the_table():
    seen = {}
    for crop, out in _axis_pairs():
        fl, rem, den = _exact(crop, out)
        ties = int(np.sum(2 * rem == den))
        if ties:
            seen[(crop, out)] = ties
            p = lc.coords32(crop, out)                                   # and float32 forms these coordinates exactly
            assert np.array_equal(p.astype(np.float64)[2 * rem == den], (fl + 0.5)[2 * rem == den])
    assert seen == lc.TIES


def test_floor_mismatch_counts_match_the_table():
    seen = {}
    for crop, out in _axis_pairs():
        fl, _, _ = _exact(crop, out)
        f32 = np.floor(lc.coords32(crop, out)).astype(np.int64)
        assert np.all((f32 == fl) | (f32 == fl - 1)), (crop, out)         # never above, never two below
        if np.any(f32 != fl):
            seen[(crop, out)] = int(np.sum(f32 == fl - 1))
    assert seen == lc.FLOOR_BELOW


def test_last_coordinate_signs_match_the_table():
    seen = {}
    for crop, out in _axis_pairs():
        if out == 1:
            continue
        last = float(lc.coords32(crop, out)[-1])
        if last != crop - 1:
            seen[(crop, out)] = 1 if last > crop - 1 else -1
    assert seen == lc.LAST_COORD
    for (crop, out), sign in lc.LAST_COORD.items():
        i0, i1, f = lc._taps32(crop, out, "tf")
        if sign > 0:            # above: i0 is the last pixel, i1 would be past it without the clamp
            assert i0[-1] == crop - 1 and i0[-1] + 1 == crop and i1[-1] == crop - 1 and 0 < f[-1] < 1e-3
        else:                   # below: the weight of the last pixel is just under 1
            assert i0[-1] == crop - 2 and i1[-1] == crop - 1 and 1 - 1e-3 < f[-1] < 1


def _label_rows(name, channels=3):
    n = STORES[lc.GROUP[name].store].n
    return [(j, r) for j, r in enumerate(lc.rows_of(name, channels)) if _valid(r.seg, n)]


def test_half_even_rounding_changes_a_label_on_every_tie_row():
    checked = 0
    for g in GROUPS:
        for j, r in _label_rows(g.name):
            if (r.box[2], g.out_hw[0]) not in lc.TIES and (r.box[3], g.out_hw[1]) not in lc.TIES:
                continue
            away, even = lc.label_with(g.store, r, g.out_hw, False), lc.label_with(g.store, r, g.out_hw, True)
            want = lc.r32_sample(g.store, r, g.out_hw, flips=False)[1]
            assert np.array_equal(away, want), (g.name, j)
            assert np.any(even != want), (g.name, j)
            checked += 1
    assert checked >= 8


@pytest.mark.parametrize("name", [g.name for g in GROUPS])
def test_unflipped_result_differs_on_every_flip_row(name):
    """Per flipped axis: with more than one output pixel and more than one crop pixel on it the flip changes image and label;
    on a degenerate axis (an output or a crop of 1) it cannot, and R32 says so."""
    g = lc.GROUP[name]
    n = STORES[g.store].n
    for j, r in enumerate(lc.rows_of(name, 3)):
        img, lab = lc.r32_sample(g.store, r, g.out_hw)
        for axis, on, crop in ((0, r.flip_ud, r.box[2]), (1, r.flip_lr, r.box[3])):
            if not on:
                continue
            off = r._replace(flip_ud=0) if axis == 0 else r._replace(flip_lr=0)
            img0, lab0 = lc.r32_sample(g.store, off, g.out_hw)
            if g.out_hw[axis] > 1 and crop > 1:
                assert not np.array_equal(img, img0), (name, j, axis)
                if _valid(r.seg, n):
                    assert not np.array_equal(lab, lab0), (name, j, axis)
            else:
                assert np.array_equal(img, img0) and np.array_equal(lab, lab0), (name, j, axis)


def test_every_clamp_row_changes_its_box():
    hw = STORES["small"].hw
    rows = lc.clamp_rows()
    kinds = set()
    for r in rows[:-1]:
        oy, ox, ch, cw = lc.clamp_box(r.box, hw)
        assert (oy, ox, ch, cw) != r.box, r.box
        assert 0 <= oy and 0 <= ox and ch >= 1 and cw >= 1 and oy + ch <= hw[0] and ox + cw <= hw[1]
        assert all(-8 <= v <= max(hw) + 12 for v in r.box)               # requests stay within a few rows of the slice
        kinds |= {k for k, hit in (("neg_off", r.box[0] < 0 or r.box[1] < 0), ("off_at_extent", r.box[0] == hw[0] or r.box[1] == hw[1]),
                                   ("off_past_extent", r.box[0] > hw[0] or r.box[1] > hw[1]), ("zero_extent", 0 in r.box[2:]),
                                   ("neg_extent", r.box[2] < 0 or r.box[3] < 0),
                                   ("past_slice", r.box[0] + r.box[2] > hw[0] or r.box[1] + r.box[3] > hw[1])) if hit}
    assert kinds == {"neg_off", "off_at_extent", "off_past_extent", "zero_extent", "neg_extent", "past_slice"}
    assert lc.clamp_box(rows[-1].box, hw) == rows[-1].box                # the last row is in bounds: the far corner pixel
    assert {(r.flip_lr, r.flip_ud) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    img, _ = lc.r32_batch("small", rows, lc.CLAMP_OUT_HW)
    assert np.isfinite(img).all() and img.std() > 0.2


# ------------------------------------------------------------------------------------------------- the references agree
@pytest.mark.parametrize("name,channels", GROUP_C)
def test_r64_agrees_with_r32(name, channels):
    """Labels are equal; the images differ by no more than the float32 coordinate error times the steepest slope of the
    normalised image, plus R32's own rounding (within the image bound of R64's exact lerp)."""
    g = lc.GROUP[name]
    im, _ = lc.store(g.store)
    step = float(np.abs(np.diff(im.astype(np.int64), axis=2)).max())
    worst = 0.0
    for j, r in enumerate(lc.rows_of(name, channels)):
        img32, lab32 = lc.r32_sample(g.store, r, g.out_hw)
        img64, lab64 = lc.r64_sample(g.store, r, g.out_hw)
        assert np.array_equal(lab32, lab64), (name, j)
        gap = float(np.abs(img32 - img64).max())
        slope = step / float(r.clip[1] - r.clip[0])
        cap = slope * (lc.coord_error(r.box[2], g.out_hw[0]) + lc.coord_error(r.box[3], g.out_hw[1])) + lc.image_bound(g.store, r.clip)
        assert gap <= cap, (name, j, gap, cap)
        worst = max(worst, gap)
    print("max |R32 - R64| {} C={}: {:.2e}".format(name, channels, worst))


def test_r64_agrees_with_r32_on_the_other_rows():
    for rows, hw, scales in ((lc.lab_scale_rows(), lc.LAB_SCALE_OUT_HW, lc.LAB_SCALES), (lc.clamp_rows(), lc.CLAMP_OUT_HW, (64,))):
        for s in scales:
            for j, r in enumerate(rows):
                img32, lab32 = lc.r32_sample("small", r, hw, s)
                img64, lab64 = lc.r64_sample("small", r, hw, s)
                assert np.array_equal(lab32, lab64), (j, s)
                assert np.abs(img32 - img64).max() <= 2e-5, j
    labs = {s: lc.r32_batch("small", lc.lab_scale_rows(), lc.LAB_SCALE_OUT_HW, s)[1] for s in lc.LAB_SCALES}
    assert labs[1][0].max() == 255 and labs[255][0].max() == 1 and labs[100][0].max() == 2 and labs[64][0].max() == 3
    assert set(np.unique(labs[1][0]).tolist()) == set(range(256))                    # the identity row sees every value


# ------------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("name", [g.name for g in GROUPS])
def test_bound_is_honest_and_sharp(name):
    """The restatement here equals R32 bit for bit; with its three lerps fused it stays inside the bound on every row; with
    the coordinate or the weight formed differently it falls outside on every full-slice row."""
    g = lc.GROUP[name]
    n = STORES[g.store].n
    for j, r in enumerate(lc.rows_of(name, 3)):
        want = lc.r32_sample(g.store, r, g.out_hw)[0]
        assert np.array_equal(lc.variant_image(g.store, r, g.out_hw, "tf"), want), (name, j)
        bound = lc.image_bound(g.store, r.clip)
        fused = float(np.abs(lc.variant_image(g.store, r, g.out_hw, "fused").astype(np.float64) - want).max())
        assert fused <= bound, (name, j, fused, bound)
        if lc.is_full(name, j) and any(_valid(s, n) for s in r.chans):
            for mode in ("recip", "fma_f"):
                err = float(np.abs(lc.variant_image(g.store, r, g.out_hw, mode).astype(np.float64) - want).max())
                print("{} row {} box {}: fused {:.2e} <= bound {:.2e} < {} {:.2e}".format(name, j, r.box, fused, bound, mode, err))
                assert err > 10 * bound, (name, j, mode, err, bound)


def test_bound_figures():
    assert lc.raw_rounding("big") == 2.0 ** -10 and lc.raw_rounding("small") == 2.0 ** -14
    assert 4.0e-7 < lc.image_bound("big", lc.rows_of("ws256", 3)[0].clip) < 5.0e-7
    assert 1.5e-6 < lc.image_bound("small", lc.rows_of("tie33", 3)[0].clip) < 2.5e-6


# ------------------------------------------------------------------------------------------------- second trip, noise
def test_second_trip_row_passes_2_pow_24():
    h, w = lc.TRIP2_HW
    assert h * w == 2 ** 24 + 4096 and (h * w + 255) // 256 > 65536                # the grid cap of 65,536 blocks is hit
    assert lc.clamp_box(lc.TRIP2_ROW.box, STORES["small"].hw) == lc.TRIP2_ROW.box


def test_u01_restatement():
    """Pinned on hand-checkable facts: [0, 1) in steps of 2^-24, seed and counter both matter, counters past 2^32 differ from
    their low words, and the first values for seed 0 (python integers, the same formula)."""
    def scalar(seed, i):
        m = (1 << 64) - 1
        z = ((i + 0x9E3779B97F4A7C15) * 0xBF58476D1CE4E5B9 + (seed << 32 | seed)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return (z >> 40) / 16777216.0
    counters = [0, 1, 2, 255, 2 ** 24, 2 ** 24 + 4095, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7]
    for seed in lc.NOISE_SEEDS:
        got = lc.u01(seed, np.array(counters, dtype=np.uint64))
        assert got.tolist() == [scalar(seed, i) for i in counters]
        assert np.all((got >= 0) & (got < 1)) and len(set(got.tolist())) == len(counters)
    u = lc.u01(123, np.arange(1 << 16, dtype=np.uint64))
    assert abs(u.mean() - 0.5) < 5e-3 and abs(u.std() - 12 ** -0.5) < 5e-3
    f = lc.noise_field(123, (2, 5, 7, 3), 0.05)
    assert f.shape == (2, 5, 7, 3) and np.abs(f).max() <= 0.05
    assert not np.array_equal(f[..., 0], f[..., 1]) and not np.array_equal(f[0], f[1])


def test_check_noise_sees_a_shared_or_truncated_counter():
    """The checker itself: a field drawn with one counter per pixel (shared across channels), per sample (shared across
    samples) or from the other seed is refused."""
    shape = (2, 4, 5, 3)
    clean = np.random.default_rng(1).random(shape).astype(F32)
    field = lc.noise_field(7, shape, 0.05)
    good = (clean.astype(np.float64) + field).astype(F32)
    real = np.ones(shape, bool)
    real[1, ..., 2] = False
    good[~real] = clean[~real]
    assert lc.check_noise(good, clean, 7, 0.05, real) <= 1.0
    per_pixel = lc.noise_field(7, shape[:3] + (1,), 0.05)
    per_sample = np.broadcast_to(lc.noise_field(7, (1,) + shape[1:], 0.05), shape)
    for wrong in (np.broadcast_to(per_pixel, shape), per_sample, lc.noise_field(8, shape, 0.05)):
        bad = (clean.astype(np.float64) + wrong).astype(F32)
        bad[~real] = clean[~real]
        with pytest.raises(AssertionError):
            lc.check_noise(bad, clean, 7, 0.05, real)
    leak = good.copy()
    leak[1, 0, 0, 2] += F32(0.01)
    with pytest.raises(AssertionError):
        lc.check_noise(leak, clean, 7, 0.05, real)
