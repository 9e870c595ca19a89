"""CPU: the slice prior of click-guided UNet3D (--slice_prior) -- the identity the kernels lean on (the 3-D
transform of seeds in one slice is dz^2 + D2), the boundary rule at the borders of the box, and the flag with its refusals."""
import argparse

import numpy as np
import pytest

import slice_prior_ref as sref

BASE_3D = "liver_3d --mode train --tag t --model UNet3D --classes Liver Tumor --im_depth 4 --im_height 32 --im_width 32".split()
BASE_EVAL = "--mode eval --tag t --model UNet3D --classes Tumor --im_depth 4 --im_height 32 --im_width 32".split()


def _masks():
    rng = np.random.default_rng(5)
    yy, xx = np.meshgrid(np.arange(23), np.arange(31), indexing="ij")
    out = {"random": rng.random((23, 31)) < 0.4, "sparse": rng.random((23, 31)) < 0.02,
           "disc": (yy - 11) ** 2 + (xx - 15) ** 2 <= 64, "ring": np.abs(np.hypot(yy - 11, xx - 15) - 8) <= 1.5,
           "one pixel": (yy == 7) & (xx == 29), "corner pixel": (yy == 0) & (xx == 0),
           "all but one": ~((yy == 22) & (xx == 30)), "touches all borders": (np.abs(yy - 11) <= 3) | (np.abs(xx - 15) <= 2),
           "checkerboard": (yy + xx) % 2 == 0, "left column": xx == 0, "far corners": ((yy == 0) & (xx == 0)) | ((yy == 22) & (xx == 30))}
    return {k: v.astype(np.uint8) for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(_masks()))
def test_3d_transform_of_one_seeded_slice_is_dz2_plus_d2(name):
    mask = _masks()[name]
    b = sref.inner_boundary(mask)
    assert b.any()
    d2 = sref.d2_brute(b)
    for depth, z0 in ((1, 0), (7, 0), (7, 3), (7, 6)):
        lit = np.rint(sref.edt3d(b, z0, depth) ** 2).astype(np.int64)            # the reference's call, literally
        dz = np.arange(depth) - z0
        np.testing.assert_array_equal(lit, dz[:, None, None] ** 2 + d2[None], err_msg=str((name, depth, z0)))
    np.testing.assert_array_equal(sref.field(mask), d2)
    # and the prior is exp(-sqrt(.) / 25) of exactly that integer
    vol = sref.prior_volume(mask, 2, 5)
    dz = np.arange(5) - 2
    np.testing.assert_allclose(vol, np.exp(-np.sqrt(dz[:, None, None] ** 2 + d2[None].astype(np.float64)) / 25), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", sorted(_masks()))
def test_boundary_rule_equals_dilation_ne_erosion(name):
    mask = _masks()[name]
    np.testing.assert_array_equal(sref.inner_boundary(mask), sref.boundary_brute(mask))


def test_boundary_rule_at_the_borders_of_the_box():
    full = np.ones((5, 6), np.uint8)
    assert not sref.inner_boundary(full).any()                                   # the border is not background
    assert (sref.field(full) == sref.SENTINEL).all() and not sref.prior_volume(full, 1, 3).any()
    assert not sref.inner_boundary(np.ones((1, 1), np.uint8)).any() and not sref.inner_boundary(np.zeros((4, 4), np.uint8)).any()
    m = full.copy()
    m[0, 0] = 0                                                                  # one background corner: its two neighbours only
    assert sorted(zip(*np.nonzero(sref.inner_boundary(m)))) == [(0, 1), (1, 0)]
    row = np.array([[1, 1, 0, 1, 1, 1, 1]], np.uint8)                            # a 1 x 7 box: no neighbour above or below
    np.testing.assert_array_equal(sref.inner_boundary(row), [[0, 1, 0, 1, 0, 0, 0]])
    np.testing.assert_array_equal(sref.field(row), [[1, 0, 1, 0, 1, 4, 9]])
    np.testing.assert_array_equal(sref.field(row.T), np.array([[1, 0, 1, 0, 1, 4, 9]]).T)
    np.testing.assert_array_equal(sref.field(row, "binary"), row)
    blob = np.zeros((6, 6), np.uint8)
    blob[1:5, 1:5] = 1                                                           # interior pixels are not boundary
    assert sref.inner_boundary(blob).sum() == 12 and not sref.inner_boundary(blob)[2:4, 2:4].any()


def test_no_click_and_binary_priors():
    mask = _masks()["disc"]
    assert not sref.prior_volume(np.zeros_like(mask), 2, 5).any()
    vol = sref.prior_volume(mask, 4, 5, "binary")
    np.testing.assert_array_equal(vol[4], mask)
    assert not vol[:4].any()
    assert not sref.prior_volume(mask, 5, 5).any() and not sref.prior_volume(mask, -1, 5).any()
    lab = np.zeros((3, 8, 8), np.uint8)
    lab[2, 2:5, 2:5] = 2
    assert sref.box_mask(lab, (0, 0, 0, 8, 8), 2, 2, 4).sum() == 9
    assert not sref.box_mask(lab, (0, 0, 0, 8, 8), 3, 2, 4).any()                # a zero-padded slice of a shallow case
    assert not sref.box_mask(lab, (0, 0, 0, 8, 8), 4, 2, 4).any()


# ------------------------------------------------------------------------------------------------- the flag
def test_flag_parses_in_both_entries_with_default_off():
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval_3d
    args, _, _ = entry.get_arguments(BASE_3D)
    assert args.slice_prior == "off" and lits3d.slice_prior(args) is None and lits3d.check_args(args) == (2, 2)
    for mode in ("boundary", "binary"):
        args, _, _ = entry.get_arguments(BASE_3D + ["--use_spatial", "--im_channel", "2", "--slice_prior", mode])
        assert args.slice_prior == mode and lits3d.slice_prior(args) == mode and lits3d.check_args(args) == (2, 2)
        ev = main_eval_3d.get_arguments(BASE_EVAL + ["--use_spatial", "--im_channel", "2", "--slice_prior", mode])
        assert ev.slice_prior == mode and main_eval_3d.check_args(ev) == 2
    assert main_eval_3d.get_arguments(BASE_EVAL).slice_prior == "off"
    with pytest.raises(SystemExit):
        entry.get_arguments(BASE_3D + ["--slice_prior", "edges"])


@pytest.mark.parametrize("extra,names", [
    (["--im_channel", "2", "--slice_prior", "boundary"], ["--slice_prior", "--use_spatial"]),
    (["--use_spatial", "--slice_prior", "boundary"], ["--slice_prior", "--im_channel"]),
    (["--use_spatial", "--im_channel", "3", "--slice_prior", "binary"], ["--slice_prior", "--im_channel"]),
    (["--use_spatial", "--im_channel", "2", "--slice_prior", "boundary", "--random_rotate", "10"],
     ["--slice_prior", "--random_rotate", "--random_deform"]),
    (["--use_spatial", "--im_channel", "2", "--slice_prior", "binary", "--random_deform", "1.5"],
     ["--slice_prior", "--random_rotate", "--random_deform"])])
def test_refusals_name_their_flags(extra, names):
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval_3d
    args, _, _ = entry.get_arguments(BASE_3D + extra)
    with pytest.raises(ValueError) as e:
        lits3d.check_args(args)
    assert all(n in str(e.value) for n in names), str(e.value)
    with pytest.raises(ValueError) as e:
        main_eval_3d.check_args(main_eval_3d.get_arguments(BASE_EVAL + extra))
    assert all(n in str(e.value) for n in names), str(e.value)


def test_what_stays_refused():
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval_3d
    for flag in ("--use_cascade", "--cascade_binary"):
        with pytest.raises(SystemExit):
            entry.get_arguments(BASE_3D + [flag])                                # liver_3d does not parse them
        ev = main_eval_3d.get_arguments(BASE_EVAL + ["--use_spatial", flag])
        with pytest.raises(NotImplementedError, match=flag) as e:
            main_eval_3d.check_args(ev)
        assert "--slice_prior" in str(e.value)                                   # and points at what is built
        both = main_eval_3d.get_arguments(BASE_EVAL + ["--use_spatial", "--im_channel", "2", "--slice_prior", "boundary", flag])
        with pytest.raises(NotImplementedError, match=flag):
            main_eval_3d.check_args(both)
    for argv in (BASE_3D + ["--im_channel", "2"], BASE_3D + ["--use_spatial", "--im_channel", "2"]):
        args, _, _ = entry.get_arguments(argv)
        with pytest.raises(ValueError, match="one channel"):                      # without a prior: as before, same message
            lits3d.check_args(args)
    with pytest.raises(ValueError, match="--slice_prior"):
        lits3d.slice_prior(argparse.Namespace(slice_prior="edges", use_spatial=True))
