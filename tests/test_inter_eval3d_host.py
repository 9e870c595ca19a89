"""CPU: the 3-D interactive evaluator's host side.  The restatement of the click step and the session loop
(inter_eval3d_ref.py) is held to what the REFERENCE ITSELF computed (tests/golden/ref_inter_eval3d.json, written by
tests/golden/make_inter_eval3d_fixtures.py from entry/main_eval_3d.py's inter_simulation_test, update_guide and compute_dice);
entry.main_eval_3d's parser takes every `main_eval_3d` line of the reference's shipped scripts and refuses what is not built by
name; the library checks the new entry points' arguments before anything is launched."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import inter_eval3d_ref as ref
import inter_eval3d_shapes as shapes
from boxsegliver_amd.entry import main_eval, main_eval_3d

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_inter_eval3d.json")) as _f:
    RECORDS = json.load(_f)
with open(os.path.join(HERE, "golden", "ref_run_scripts.json")) as _f:
    EVAL_LINES = [(script, argv) for script, calls in sorted(json.load(_f)["scripts"].items()) for which, argv in calls
                  if which == "main_eval_3d"]
SHAPES = ([6, 20, 24], [12, 40, 48], [20, 64, 70])


def _masks(rec):
    return shapes.build(rec["shape"], rec["pred"]), shapes.build(rec["shape"], rec["ref"])


def _session(rec):
    shape = rec["shape"]
    if "pred" in rec:
        def predictor(fg, bg):
            return shapes.build(shape, rec["pred"])
    else:
        def predictor(fg, bg):
            return shapes.ball_prediction(shape, fg, bg, rec["r_fg"], rec["r_bg"])
    return ref.session(shapes.build(shape, rec["ref"]), predictor, rec["inter_thresh"], rec["max_iter"])


def test_the_records_hold_every_situation():
    """Asserted on the records (and the volumes they describe) before any device is asked."""
    singles, sessions = RECORDS["singles"], RECORDS["sessions"]
    assert sorted({tuple(r["shape"]) for r in singles}) == sorted(tuple(s) for s in SHAPES)
    placed = [r["kind"] for r in singles if not r["fallback"]]
    assert len(placed) >= 18 and set(placed) == {0, 1}
    fallback = [ref.click(*_masks(r))["kind"] for r in singles if r["fallback"]]
    assert len(fallback) >= 6 and set(fallback) == {0, 1}
    assert len(sessions) == 6 and sum(len(s["rounds"]) for s in sessions) >= 6
    assert all(s["stop"] == "fallback" for s in sessions)              # each was followed up to its first fallback round
    ties = elsewhere = 0
    halves_even, halves_odd = [0, 0, 0], [0, 0, 0]
    for r in singles:
        if r["fallback"]:
            continue
        pred, lab = _masks(r)
        err = pred.astype(bool) ^ lab.astype(bool)
        res, n = ndi.label(err, ndi.generate_binary_structure(3, 1))
        sizes = np.bincount(res.ravel())[1:]
        best = int(np.argmax(sizes)) + 1
        coords = np.nonzero(res == best)
        lin = np.ravel_multi_index(coords, err.shape)
        if (sizes == sizes.max()).sum() == 2:
            other = [i + 1 for i in range(n) if sizes[i] == sizes.max() and i + 1 != best][0]
            assert lin[0] < np.ravel_multi_index(np.nonzero(res == other), err.shape)[0]      # the smaller root
            assert res[tuple(r["click"])] == best                                             # and the reference clicked there
            ties += 1
        for axis, s in enumerate(coords):
            if 2 * int(s.sum()) % s.size == 0 and (2 * int(s.sum()) // s.size) % 2 == 1:      # a mean at exactly x.5
                if (int(s.sum()) // s.size) % 2 == 0:
                    halves_even[axis] += 1
                else:
                    halves_odd[axis] += 1
        if res[tuple(r["click"])] != best:
            elsewhere += 1                                                                     # err is set, in another component
    assert ties >= 1 and min(halves_even) >= 1 and min(halves_odd) >= 1 and elsewhere >= 1
    assert RECORDS["repeat"]["stop"] == "repeat" and sum(RECORDS["repeat"]["num_iter"]) == len(RECORDS["repeat"]["rounds"]) + 1


@pytest.mark.parametrize("rec", RECORDS["singles"], ids=lambda r: "{}-{}x{}x{}".format(r["name"], *r["shape"]))
def test_restatement_equals_the_reference_click(rec):
    got = ref.click(*_masks(rec))
    assert got["fallback"] == rec["fallback"] and not got["empty"]
    if not rec["fallback"]:
        assert list(got["click"]) == rec["click"] and got["kind"] == rec["kind"]
        assert got["click"] == got["cand"]


@pytest.mark.parametrize("rec", RECORDS["sessions"] + [RECORDS["repeat"]],
                         ids=lambda r: "{}x{}x{}-{}".format(*(r["shape"] + [r.get("r_fg", "fixed")])))
def test_restatement_equals_the_reference_session(rec):
    rounds, stop, num_iter = _session(rec)
    for want, got in zip(rec["rounds"], rounds):
        assert list(got[0]) == want["click"] and got[1] == want["kind"] and not got[2] and list(got[3]) == want["counts"]
    if rec["stop"] == "fallback":                      # the reference was followed up to the round that asks for the skeleton
        assert len(rounds) > len(rec["rounds"]) and rounds[len(rec["rounds"])][2]
    else:
        assert stop == rec["stop"] and len(rounds) == len(rec["rounds"]) and num_iter == rec["num_iter"]


def test_fallback_rule_on_a_hand_checked_shell():
    """A 5 x 5 x 5 block with its centre missing: the mean is the hole.  Every voxel of the block's rim is 1 from the outside
    and the hole's six neighbours 1 from the hole; the other 20 voxels of the inner 3 x 3 x 3 are 2 from both.  Nearest to the
    mean among those are the twelve edge voxels at squared distance 2, and the first of them in (z, y, x) order wins."""
    lab = shapes.build((9, 9, 9), [["+", "box", 2, 7, 2, 7, 2, 7], ["-", "box", 4, 5, 4, 5, 4, 5]])
    got = ref.click(np.zeros_like(lab), lab)
    assert got["fallback"] and got["cand"] == (4, 4, 4) and got["click"] == (3, 3, 4) and got["kind"] == 0
    assert got["area"] == 124 and got["root"] == (2 * 9 + 2) * 9 + 2 and got["n_comp"] == 1
    # the cap: with distances capped at 1 every voxel ties, the nearest to the mean are the hole's six neighbours
    got = ref.click(lab, np.zeros_like(lab), cap=1)
    assert got["fallback"] and got["click"] == (3, 4, 4) and got["kind"] == 1
    # the border counts as non-error: a block that fills the volume is 3 deep at most (5 slices)
    full = np.ones((5, 7, 9), np.uint8)
    full[2, 3, 4] = 0
    got = ref.click(np.zeros_like(full), full)
    assert got["fallback"] and got["cand"] == (2, 3, 4) and int(ref.city_block(full.astype(bool)).max()) == 3     # e.g. (2, 2, 2): 3 from three faces and from the hole
    assert ref.round_half_even_div(9, 2) == 4 and ref.round_half_even_div(11, 2) == 6 and ref.round_half_even_div(7, 3) == 2


def test_table_row_of_the_restatement():
    lab = shapes.build((6, 20, 24), shapes.two_ellipsoids((6, 20, 24)))
    row, kind, click, appended = ref.table_row(np.zeros_like(lab), lab, prev=(2, 9, 11), have=(0, 0), k=1)
    assert kind == 0 and click == (2, 9, 11) and appended and row[14] == 1 and row[16] == 1 and row[17] == 1
    assert list(row[9:12]) == [2, 9, 11] and row[1] == int(lab.sum()) and row[0] == row[2] == 0
    row, kind, click, appended = ref.table_row(np.zeros_like(lab), lab, have=(1, 0), k=1)
    assert not appended and row[16] == 0 and row[14] == 0
    row, kind, click, appended = ref.table_row(lab, lab)
    assert click is None and kind == -1 and row[15] == 1 and list(row[5:13]) == [-1] * 8


def _argv(argv):
    return ["Tumor" if a == "NF" else a for a in argv] + ["--lits_root", "data/LiTS"]


def test_every_main_eval_3d_line_of_the_shipped_scripts_parses():
    assert len(EVAL_LINES) == 17
    refused = {}
    for script, argv in EVAL_LINES:
        args = main_eval_3d.get_arguments(_argv(argv))
        assert args.tag == os.path.basename(script)[:-3] and args.mode == "eval" and args.lits_root == "data/LiTS"
        assert (args.inter_thresh, args.max_iter, args.infer_set, args.save_path, args.save_subdir) == (0.9, 20, "eval", "prediction", "prediction")
        assert not args.eval_final and args.ckpt_path is None and not args.test and args.seed == 1234
        assert args.eval_overlap == 0.5 and args.eval_window_weight == "uniform" and args.eval_box_from is None
        assert args.use_spatial == ("202_unetinter" in script)
        with pytest.raises((NotImplementedError, ValueError)) as e:    # every shipped line asks for something that is not built
            main_eval_3d.check_args(args)
        refused[script] = str(e.value)
        # the same line in windows of the training depth, without the unbuilt flags, is taken
        built = [a for a in _argv(argv) if a not in ("--use_cascade", "--cascade_binary", "-ds")]
        built[built.index("--im_depth") + 1] = "10"
        built[built.index("--im_channel") + 1] = "1"                   # the cascade lines count its prediction as a channel
        assert main_eval_3d.check_args(main_eval_3d.get_arguments(built)) == 2                 # --classes Tumor: stored label >= 2
    assert sum("--use_cascade" in v for v in refused.values()) == 3 and sum("--downsampling" in v for v in refused.values()) == 7
    assert sum("--im_depth" in v for v in refused.values()) == 7


@pytest.mark.parametrize("flag,name,exc", [("--use_cascade", "--use_cascade", NotImplementedError),
                                           ("--cascade_binary", "--cascade_binary", NotImplementedError),
                                           ("-ds", "--downsampling", NotImplementedError), ("--test", "--test", NotImplementedError),
                                           ("--save_predict", "--save_predict", NotImplementedError),
                                           ("--im_depth -1", "--im_depth", ValueError), ("--im_depth 0", "--im_depth", ValueError),
                                           ("--max_iter 65", "--max_iter", ValueError), ("--max_iter -1", "--max_iter", ValueError),
                                           ("--infer_set test", "--infer_set", ValueError)])
def test_refusals_name_their_flag_before_anything_is_loaded(flag, name, exc, tmp_path):
    argv = ("--mode eval --tag t --model UNet3D --classes Tumor --im_depth 4 --im_height 32 --im_width 32 --use_spatial --lits_root {} "
            "--model_dir {}").format(tmp_path / "nowhere", tmp_path / "run").split() + flag.split()
    args = main_eval_3d.get_arguments(argv)
    with pytest.raises(exc, match=name):
        main_eval_3d.run(args)                                     # no dataset, no checkpoint, no device: none is reached
    assert not (tmp_path / "run").exists()


def test_accepted_values_and_object_labels():
    base = "--mode eval --tag t --model UNet3D --im_depth 4 --im_height 32 --im_width 32 --use_spatial".split()
    ok = main_eval_3d.get_arguments(base + ["--classes", "Tumor", "--max_iter", "64", "--infer_set", "train"])
    assert main_eval_3d.check_args(ok) == 2
    assert main_eval_3d.check_args(main_eval_3d.get_arguments(base + ["--classes", "Liver", "--max_iter", "0"])) == 1
    assert main_eval_3d.check_args(main_eval_3d.get_arguments(base + ["--classes", "Liver", "Tumor"])) == 2
    with pytest.raises(ValueError, match="--eval_overlap"):
        main_eval_3d.check_args(main_eval_3d.get_arguments(base + ["--classes", "Tumor", "--eval_overlap", "1.0"]))
    with pytest.raises(ValueError, match="--stddev"):
        main_eval_3d.check_args(main_eval_3d.get_arguments(base + ["--classes", "Tumor", "--stddev", "1", "3"]))


def test_liver_3d_still_refuses_guided_evaluation_and_points_here():
    import argparse

    from boxsegliver_amd.data import lits3d
    with pytest.raises(NotImplementedError, match="--mode eval with --use_spatial") as e:
        lits3d.check_args(argparse.Namespace(classes=["Liver", "Tumor"], mode="eval", use_spatial=True, im_depth=4, im_height=32,
                                             im_width=32))
    assert "main_eval_3d" in str(e.value)
    assert lits3d.check_args(argparse.Namespace(classes=["Liver", "Tumor"], mode="train", use_spatial=True, im_depth=4,
                                                im_height=32, im_width=32)) == (2, 2)


def test_dice_is_compute_dice():
    assert main_eval_3d.dice is main_eval.dice
    assert main_eval_3d.dice(3, 5, 2) == ref.dice(3, 5, 2) == main_eval.dice(3, 5, 2) == (4 + 1e-8) / (8 + 1e-8)
    assert main_eval_3d.dice(0, 0, 0) == 1.0


# ------------------------------------------------------------------------------------------------- the library
def _desc(base=0, depth=64, n_slices=1000, src=(512, 512), k=20, cap=255, lab_scale=64, obj=2):
    from boxsegliver_amd import _abi
    return _abi.InterClick3dDesc(case_base=base, depth=depth, n_slices=n_slices, src_h=src[0], src_w=src[1], lab_scale=lab_scale,
                                 obj_label=obj, K=k, dist_cap=cap)


def _gdesc(n=4, d=10, h=256, w=256, src=(512, 512), g=2, gaussian=1, stddev=(1, 3, 3), norm=1.0):
    from boxsegliver_amd import _abi
    return _abi.Lits3dClicksDesc(N=n, D=d, H=h, W=w, n_slices=1, src_h=src[0], src_w=src[1], lab_scale=64, obj_label=2, margin=3,
                                 step=10, band=40, max_clicks=5, G=g, gaussian=gaussian, stddev=(ctypes.c_float * 3)(*stddev),
                                 euclid_norm=norm)


def test_the_library_exports_the_new_entry_points_and_checks_their_arguments():
    """Every refusal returns before anything is launched."""
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_inter_click3d_ws_bytes", "unetk_inter_click3d", "unetk_click_guide3d_list"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.unetk_abi_version() == 10 and _abi.INTER3D_TAB_COLS == ref.TAB_COLS == 20                  # additive
    d = _desc()
    vox = 64 * 512 * 512
    nbytes = lib.unetk_inter_click3d_ws_bytes(ctypes.byref(d))
    assert nbytes == 256 + 256 + 9 * vox and nbytes % 16 == 0          # header, info; err bytes, labels and sizes per voxel
    p = ctypes.c_void_p(1 << 20)                                       # never dereferenced: the calls return first
    call = lib.unetk_inter_click3d
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, p, p, p, nbytes - 1, None) == -3                    # UNETK_E_WORKSPACE
    assert call(ctypes.byref(d), None, p, -1, -1, -1, p, p, p, p, nbytes, None) == -1                     # UNETK_E_BADARG
    assert call(ctypes.byref(d), p, p, -1, -1, -1, None, p, p, p, nbytes, None) == -1
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, None, p, p, nbytes, None) == -1
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, p, None, p, nbytes, None) == -1
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, p, p, None, nbytes, None) == -1
    odd, off8 = ctypes.c_void_p((1 << 20) + 2), ctypes.c_void_p((1 << 20) + 8)
    assert call(ctypes.byref(d), p, p, -1, -1, -1, odd, p, p, p, nbytes, None) == -1
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, odd, p, p, nbytes, None) == -1
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, p, odd, p, nbytes, None) == -1
    assert call(ctypes.byref(d), p, p, -1, -1, -1, p, p, p, off8, nbytes, None) == -1
    for bad in (_desc(src=(1025, 512)), _desc(src=(512, 1025)), _desc(k=65), _desc(depth=4097, src=(16, 16)),
                _desc(depth=2048, src=(1024, 1024))):                  # the last: depth * src_h * src_w = 2^31
        assert lib.unetk_inter_click3d_ws_bytes(ctypes.byref(bad)) == 0
        assert call(ctypes.byref(bad), p, p, -1, -1, -1, p, p, p, p, 1 << 40, None) == -2                 # UNETK_E_UNSUPPORTED
    assert lib.unetk_inter_click3d_ws_bytes(ctypes.byref(_desc(depth=2047, src=(1024, 1024), k=64))) > 0
    assert lib.unetk_inter_click3d_ws_bytes(ctypes.byref(_desc(depth=4096, src=(16, 16)))) > 0
    for bad in (_desc(depth=0), _desc(n_slices=0), _desc(k=0), _desc(cap=0), _desc(cap=256), _desc(obj=0), _desc(lab_scale=0),
                _desc(src=(0, 512))):
        assert lib.unetk_inter_click3d_ws_bytes(ctypes.byref(bad)) == 0
        assert call(ctypes.byref(bad), p, p, -1, -1, -1, p, p, p, p, 1 << 40, None) == -1
    # the guide from lists
    g = _gdesc()
    glist = lib.unetk_click_guide3d_list
    for k in (0, -1, 65):
        assert glist(ctypes.byref(g), p, p, p, k, p, None) == -1
    assert glist(ctypes.byref(g), p, p, p, 20, None, None) == -1
    assert glist(ctypes.byref(g), p, None, p, 20, p, None) == -1
    assert glist(ctypes.byref(g), p, p, odd, 20, p, None) == -1
    assert glist(ctypes.byref(_gdesc(g=3)), p, p, p, 20, p, None) == -1
    assert glist(ctypes.byref(_gdesc(stddev=(1, 0, 3))), p, p, p, 20, p, None) == -1
    assert glist(ctypes.byref(_gdesc(gaussian=0, norm=0.0)), p, p, p, 20, p, None) == -1
    assert glist(ctypes.byref(_gdesc(n=1, d=2048, h=1024, w=1024)), p, p, p, 20, p, None) == -2            # D*H*W = 2^31
    for name in ("unetk_click_guide3d", "unetk_inter_click", "unetk_click_guide_list"):                    # still there
        assert hasattr(lib, name)
