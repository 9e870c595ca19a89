"""Host: `liver_3d --z_spacing MM` -- the flag and its refusals, the crop depth per case and its errors, a
sampler whose draws do not notice the flag, the window tiling with cd-deep windows, the slice spacing of a --mode infer volume
read through a transposed header, and the restatement (lits3d_zspace_ref.py) against the plain ones where crop depth == D."""
import numpy as np
import pytest

import eval3d_ref
import eval3d_weighted_ref as wref
import lits3d_ref as ref
import lits3d_zspace_ref as zref

BASE = ("liver_3d --tag t --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 --im_width 32 "
        "--batch_size 2 --evaluator Volume").split()
HW = (ref.H, ref.W)


def _args(mode="train", extra=()):
    from boxsegliver_amd.entry import main as entry
    return entry.get_arguments(BASE + ["--mode", mode] + list(extra))[0]


def _meta(spacings=None):
    cases = ref.make_cases()
    spacings = [2.5] * len(cases) if spacings is None else spacings
    return [{"PID": pid, "size": [im.shape[0], ref.H, ref.W], "spacing": [sz, 0.8, 0.8]}
            for pid, ((im, _), sz) in enumerate(zip(cases, spacings))]


def _sampler(z_spacing=None, spacings=None, seed=7, shape=(4, 16, 20), **kw):
    from boxsegliver_amd.data import lits3d
    _, lb, base = ref.stack_store(ref.make_cases())
    counts = (lb // 64 >= 2).sum(axis=(1, 2))
    offset = {pid: int(b) for pid, b in enumerate(base)}
    return lits3d.PatchSampler(_meta(spacings), offset, counts, 4, shape, HW, tumor_percent=0.5, seed=seed, z_spacing=z_spacing, **kw)


# ------------------------------------------------------------------------------------------------- entries and flag
def test_new_entries_are_bound_and_the_abi_stays():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    assert _abi.ABI_VERSION == 10 and lib.unetk_abi_version() == 10
    for name in ("unetk_lits_patch3d_z", "unetk_eval3d_accumulate_z", "unetk_eval3d_accumulate_wz"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_the_flag_is_off_by_default_and_checked():
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main_eval_3d
    assert _args().z_spacing is None and lits3d.z_spacing(_args()) is None
    for mode, extra in (("train", []), ("eval", ["--eval_in_patches"]), ("infer", [])):
        a = _args(mode, extra + ["--z_spacing", "1.5"])
        assert lits3d.z_spacing(a) == 1.5 and lits3d.check_args(a) == (2, 2)
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(ValueError, match="--z_spacing"):
            lits3d.check_args(_args(extra=["--z_spacing", bad]))
    with pytest.raises(SystemExit):                                 # the interactive evaluator needs --use_spatial: no such flag
        main_eval_3d.build_parser().parse_args(["--z_spacing", "1.5"])


@pytest.mark.parametrize("flag,extra", [
    ("--use_spatial", ["--use_spatial"]),
    ("--slice_prior", ["--use_spatial", "--slice_prior", "boundary", "--im_channel", "2"]),
    ("--hard_neg_clicks", ["--use_spatial", "--hard_neg_clicks", "--hard_neg_from", "negs"]),
    ("--random_rotate", ["--random_rotate", "15"]),
    ("--random_deform", ["--random_deform", "1.5"])])
def test_what_is_not_resampled_along_z_is_refused_by_name(flag, extra):
    from boxsegliver_amd.data import lits3d
    lits3d.check_args(_args(extra=extra))                           # served without the flag
    with pytest.raises(NotImplementedError, match="--z_spacing with {} is not built".format(flag)):
        lits3d.check_args(_args(extra=extra + ["--z_spacing", "1.0"]))


def test_hard_negative_patches_stay_allowed():
    from boxsegliver_amd.data import lits3d
    a = _args(extra=["--z_spacing", "1.0", "--hard_neg_from", "negs", "--hard_neg_patches", "0.5", "--tumor_percent", "0.5"])
    assert lits3d.check_args(a) == (2, 2)


# ------------------------------------------------------------------------------------------------- crop depth
@pytest.mark.parametrize("d,mm,sz,want", [(10, 2.5, 2.5, 10), (10, 1.0, 1.0, 10), (10, 5.0, 2.5, 19), (10, 1.0, 2.0, 5), (10, 1.0, 5.0, 3),
                                          (10, 2.5, 0.7, 33), (10, 0.5, 5.0, 2), (10, 0.1, 5.0, 1), (1, 3.0, 0.5, 1), (4, 2.5, 1.25, 7),
                                          (4, 2.5, 5.0, 3), (96, 1.0, 0.5, 191), (2, 1.0, 2.0, 1), (2, 3.0, 2.0, 3)])
def test_crop_depth(d, mm, sz, want):
    """cd = int(round((D - 1) MM / sz)) + 1, at least 1; sz == MM gives D.  (10, 1, 2): round(4.5) = 4, Python's rounding to
    even; (2, 1, 2): round(0.5) = 0; (2, 3, 2): round(1.5) = 2."""
    from boxsegliver_amd.data import lits3d
    assert lits3d.crop_depth(d, mm, sz) == want == max(int(round((d - 1) * mm / sz)) + 1, 1)


def test_a_case_without_a_positive_spacing_and_a_crop_beyond_31_bits_raise():
    from boxsegliver_amd.data import lits3d
    meta = _meta([2.5, 1.25, 5.0, 2.5])
    np.testing.assert_array_equal(lits3d.crop_depths(meta, 4, 2.5, HW), [4, 7, 3, 4])
    for bad in (0.0, -2.5, float("nan"), float("inf"), None, "thick"):
        broken = _meta()
        broken[2]["spacing"] = [bad, 0.8, 0.8]
        with pytest.raises(ValueError, match="case 2 "):
            lits3d.crop_depths(broken, 4, 2.5, HW)
    for spacing in (None, [], 2.5):
        broken = _meta()
        broken[1]["spacing"] = spacing
        with pytest.raises(ValueError, match="case 1 "):
            lits3d.crop_depths(broken, 4, 2.5, HW)
    del broken[1]["spacing"]
    with pytest.raises(ValueError, match="case 1 "):                # the sampler looks the depths up when it is built
        lits3d.PatchSampler(broken, {p: 0 for p in range(4)}, np.ones(35), 4, (4, 16, 20), HW, z_spacing=2.5)
    lits3d.PatchSampler(broken, {p: 0 for p in range(4)}, np.ones(35), 4, (4, 16, 20), HW)       # without the flag nobody reads it
    # max(cd) * src_h * src_w >= 2^31: before anything is launched, naming the case
    thin = _meta([2.5, 2.5, 2.5, 1e-6])
    with pytest.raises(ValueError, match="case 3 .*31-bit"):
        lits3d.crop_depths(thin, 4, 2.5, HW)
    limit = -(-(1 << 31) // (ref.H * ref.W))
    lits3d.check_crop_limit([limit - 1], HW)
    with pytest.raises(ValueError, match="31-bit"):
        lits3d.check_crop_limit([3, limit], HW)


# ------------------------------------------------------------------------------------------------- the sampler
def test_the_flag_draws_nothing():
    """Same seed: draw() and table() are identical with and without the flag, batch after batch; the crop depths are looked up
    from the drawn cases and travel beside the table."""
    from boxsegliver_amd import _abi
    spacings = [2.5, 1.25, 5.0, 0.7]
    plain, flagged = _sampler(), _sampler(z_spacing=2.5, spacings=spacings)
    assert plain.zcrop is None and plain.crop_depth_rows(plain.draw()) is None
    plain = _sampler()
    np.testing.assert_array_equal(flagged.zcrop, [4, 7, 3, 12])
    assert flagged.zcrop.dtype == np.int32 and flagged.zcrop_max == 12
    for _ in range(5):
        a, b = plain.draw(), flagged.draw()
        assert sorted(a) == sorted(b)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key])
        ta, tb = plain.table(a), flagged.table(b)
        np.testing.assert_array_equal(ta, tb)
        assert tb.shape == (4, _abi.LITS3D_TAB_COLS)
        rows = flagged.crop_depth_rows(b)
        assert rows.dtype == np.int32 and rows.shape == (4,) and rows.flags.c_contiguous
        np.testing.assert_array_equal(rows, np.array([4, 7, 3, 12])[b["case"]])
    assert plain.rng.random() == flagged.rng.random()               # the generators are where they were
    # evaluation samplers take the flag too (the online evaluation inside --mode train)
    ev = _sampler(z_spacing=2.5, spacings=spacings, training=False)
    np.testing.assert_array_equal(ev.zcrop, [4, 7, 3, 12])


# ------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("depth,cd,overlap", [(12, 3, 0.5), (12, 9, 0.5), (12, 4, 0.0), (13, 4, 0.0), (5, 8, 0.5), (9, 9, 0.75), (75, 19, 0.5),
                                              (75, 19, 0.9), (7, 1, 0.5), (200, 33, 0.25)])
def test_windows_of_the_crop_depth_cover_every_slice(depth, cd, overlap):
    from boxsegliver_amd.data import lits3d
    starts = lits3d.window_starts(depth, cd, overlap)
    covered = np.zeros(depth, int)
    for a in starts:
        assert 0 <= a and (a + cd <= depth or a == 0)
        covered[a:a + cd] += 1
    assert covered.min() >= 1 and starts == sorted(set(starts))
    # eval_tables tiles z with them; the kernels' clamp gives the start back from the row's centre
    store = eval3d_ref.HostStore()
    case = {"PID": 0, "size": [ref.DEPTHS[0], ref.H, ref.W]}
    if depth == ref.DEPTHS[0]:
        assert lits3d.eval_windows(HW, (4, 16, 20), cd) == (cd, 18, 22) and lits3d.eval_windows(HW, (4, 16, 20)) == (4, 18, 22)
        tabs = list(lits3d.eval_tables(case, store, (4, 16, 20), overlap, [(0, 0, 0)], 7, cd=cd))
        tab = np.concatenate(tabs)
        z1 = sorted({zref.crop_box(r[2:5], r[5:7], cd, depth, HW)[0] for r in tab})
        assert z1 == starts
        assert lits3d.table_box(tab, (4, 16, 20), depth, HW, cd=cd) == (0, depth, 0, ref.H, 0, ref.W)
        for t in tabs:
            assert lits3d.table_box(t, (4, 16, 20), depth, HW, cd=cd) == zref.union_box(t, [cd] * len(t), depth, HW)
        plain = np.concatenate(list(lits3d.eval_tables(case, store, (cd, 16, 20), overlap, [(0, 0, 0)], 7)))
        np.testing.assert_array_equal(tab, plain)                    # the rows of a run whose --im_depth is cd


# ------------------------------------------------------------------------------------------------- --mode infer
def test_infer_reads_the_spacing_of_the_file_axis_that_becomes_z(tmp_path):
    from boxsegliver_amd.data import lits3d, nii_kits
    size, spacing = [5, 6, 7], [2.5, 0.8, 0.7]                       # (d, h, w), (sz, sy, sx)
    straight = nii_kits.header_from_meta(size, spacing)
    sform = np.zeros((3, 4))
    sform[0, 2], sform[1, 1], sform[2, 0] = -0.7, -0.8, 2.5          # file axis 0 runs along world z
    turned = nii_kits.Nifti1Header((5, 6, 7), np.int16, (2.5, 0.8, 0.7), sform=sform)
    for name, header, axis in (("straight", straight, 2), ("turned", turned, 0)):
        path = tmp_path / "{}.nii".format(name)
        nii_kits.save_flat(np.zeros(5 * 6 * 7, np.int16), header.shape, header, path)
        plan = lits3d.infer_plan(path)
        assert plan["shape"] == (5, 6, 7) and list(plan["trans_bk"]).index(0) == axis
        assert lits3d.infer_spacing(path, plan) == np.float32(2.5)
        assert lits3d.crop_depth(4, 2.5, lits3d.infer_spacing(path, plan)) == 4
    assert turned.pixdim[2] != 2.5                                   # pixdim[3] of the turned file is not its slice spacing
    for bad in (0.0, -2.5, float("nan")):
        broken = nii_kits.Nifti1Header((5, 6, 7), np.int16, (bad, 0.8, 0.7), sform=sform)
        plan = dict(header=broken, trans_bk=nii_kits.file_orientation(broken)[0], case="turned")
        with pytest.raises(ValueError, match="turned.nii.*pixdim\\[1\\]"):
            lits3d.infer_spacing(tmp_path / "turned.nii", plan)


# ------------------------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_equals_the_plain_ones_at_the_output_depth():
    cases = ref.make_cases()
    shape = (4, 12, 10)
    for ci, centre in ((0, (6, 19, 23)), (2, (4, 39, 0)), (0, (0, 0, 0))):
        im, lb = cases[ci]
        for flips in ((0, 0, 0), (1, 0, 1)):
            want = ref.patch(im, lb, centre, (16, 13), shape, flips)
            got = zref.patch(im, lb, centre, (16, 13), shape, 4, flips=flips)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b)
            # gamma: the same function on the same values; numpy's float64 sums depend on the memory layout of their argument
            want = ref.patch(im, lb, centre, (16, 13), shape, flips, gamma=0.8)[0]
            np.testing.assert_allclose(zref.patch(im, lb, centre, (16, 13), shape, 4, flips=flips, gamma=0.8)[0], want, rtol=0, atol=1e-12)
    store = eval3d_ref.HostStore(cases)
    tab = np.stack([ref.table_row(store.offset[2], 5, c, (13, 11), f) for c, f in (((2, 17, 21), (0, 0, 0)), ((4, 39, 0), (1, 1, 1)))])
    probs = np.random.default_rng(3).random((2,) + shape + (2,))
    s = zref.accumulate(tab, [4, 4], probs, shape, 5, HW)
    acc, cnt = eval3d_ref.accumulate(tab, probs, shape, 5, HW)
    np.testing.assert_array_equal(s.acc, acc)
    np.testing.assert_array_equal(s.hits, cnt)
    tables = tuple(np.random.default_rng(5).uniform(0.2, 1, n).astype(np.float32) for n in shape)
    sw, w = zref.accumulate(tab, [4, 4], probs, shape, 5, HW, tables), wref.accumulate(tab, probs, tables, shape, 5, HW)
    np.testing.assert_array_equal(sw.acc, w.acc)
    np.testing.assert_array_equal(sw.wsum, w.wsum)
    np.testing.assert_array_equal(sw.wmax, w.wmax)
    # and a resampled row is another patch: 9 slices squeezed into 4, the first and the last slice kept
    im, lb = cases[0]
    got = zref.patch(im, lb, (6, 19, 23), (12, 10), shape, 9)
    wide = ref.patch(im, lb, (6, 19, 23), (12, 10), (9, 12, 10))
    assert (got[2], got[3]) == (wide[2], wide[3])                    # the statistics of the 9-slice crop
    np.testing.assert_array_equal(got[0][[0, 3]], wide[0][[0, 8]])
    np.testing.assert_array_equal(got[1][[0, 3]], wide[1][[0, 8]])
