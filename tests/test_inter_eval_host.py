"""CPU: the interactive evaluator's host side.  The restatement of the click step and the session loop
(inter_eval_ref.py) is held to what the REFERENCE ITSELF computed (tests/golden/ref_inter_eval.json, written by
tests/golden/make_inter_eval_fixtures.py from entry/main_eval.py's inter_simulation_test, update_guide and compute_dice);
entry.main_eval's parser takes every `main_eval` line of the reference's shipped scripts, refuses what is not built by name,
and plans the mirrors as run_TTA does."""
import json
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import inter_eval_ref as ref
import inter_eval_shapes as shapes
from boxsegliver_amd.entry import main_eval

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_inter_eval.json")) as _f:
    RECORDS = json.load(_f)
with open(os.path.join(HERE, "golden", "ref_run_scripts.json")) as _f:
    EVAL_LINES = [(script, argv) for script, calls in sorted(json.load(_f)["scripts"].items()) for which, argv in calls
                  if which == "main_eval"]


def _masks(rec):
    return shapes.build(rec["shape"], rec["pred"]), shapes.build(rec["shape"], rec["ref"])


def _session(rec):
    shape = rec["shape"]
    if "pred" in rec:
        def predictor(fg, bg):
            return shapes.build(shape, rec["pred"])
    else:
        def predictor(fg, bg):
            return shapes.disc_prediction(shape, fg, bg, rec["r_fg"], rec["r_bg"])
    return ref.session(shapes.build(shape, rec["ref"]), predictor, rec["inter_thresh"], rec["max_iter"])


def test_the_records_hold_every_situation():
    """Asserted on the records (and the masks they describe) before any device is asked."""
    singles, sessions = RECORDS["singles"], RECORDS["sessions"]
    pinned = [(r["kind"]) for r in singles if not r["fallback"]] + [q["kind"] for s in sessions for q in s["rounds"]]
    assert len(pinned) >= 20 and set(pinned) == {0, 1}
    fallback = [ref.click(*_masks(r))["kind"] for r in singles if r["fallback"]]
    fallback += [_session(s)[0][len(s["rounds"])][1] for s in sessions if s["stop"] == "fallback"]
    assert len(fallback) >= 10 and set(fallback) == {0, 1}
    ties = halves_even = halves_odd = elsewhere = 0
    for r in singles:
        if r["fallback"]:
            continue
        pred, lab = _masks(r)
        err = pred.astype(bool) ^ lab.astype(bool)
        res, n = ndi.label(err)
        sizes = np.bincount(res.ravel())[1:]
        best = int(np.argmax(sizes)) + 1
        ys, xs = np.nonzero(res == best)
        if (sizes == sizes.max()).sum() == 2:
            other = [i + 1 for i in range(n) if sizes[i] == sizes.max() and i + 1 != best][0]
            oy, ox = np.nonzero(res == other)
            assert ys[0] * err.shape[1] + xs[0] < oy[0] * err.shape[1] + ox[0]            # the smaller root
            assert res[r["click"][0], r["click"][1]] == best                               # and the reference clicked there
            ties += 1
        for s in (ys, xs):
            if 2 * int(s.sum()) % s.size == 0 and (2 * int(s.sum()) // s.size) % 2 == 1:   # a mean at exactly x.5
                if (int(s.sum()) // s.size) % 2 == 0:
                    halves_even += 1
                else:
                    halves_odd += 1
        if res[r["click"][0], r["click"][1]] != best:
            elsewhere += 1                                                                  # err is set, in another component
    assert ties >= 1 and halves_even >= 1 and halves_odd >= 1 and elsewhere >= 1
    assert RECORDS["repeat"]["stop"] == "repeat" and sum(RECORDS["repeat"]["num_iter"]) == len(RECORDS["repeat"]["rounds"]) + 1


@pytest.mark.parametrize("rec", RECORDS["singles"], ids=lambda r: "{}-{}x{}".format(r["name"], *r["shape"]))
def test_restatement_equals_the_reference_click(rec):
    got = ref.click(*_masks(rec))
    assert got["fallback"] == rec["fallback"] and not got["empty"]
    if not rec["fallback"]:
        assert list(got["click"]) == rec["click"] and got["kind"] == rec["kind"]
        assert got["click"] == got["cand"]


@pytest.mark.parametrize("rec", RECORDS["sessions"] + [RECORDS["repeat"]],
                         ids=lambda r: "{}x{}-{}".format(r["shape"][0], r["shape"][1], r.get("r_fg", "fixed")))
def test_restatement_equals_the_reference_session(rec):
    rounds, stop, num_iter = _session(rec)
    for want, got in zip(rec["rounds"], rounds):
        assert list(got[0]) == want["click"] and got[1] == want["kind"] and not got[2] and list(got[3]) == want["counts"]
    if rec["stop"] == "fallback":                      # the reference was followed up to the round that asks for the skeleton
        assert len(rounds) > len(rec["rounds"]) and rounds[len(rec["rounds"])][2]
    else:
        assert stop == rec["stop"] and len(rounds) == len(rec["rounds"]) and num_iter == rec["num_iter"]


def test_fallback_rule_on_a_hand_checked_ring():
    """A 5 x 5 block with its centre missing: the mean is the hole.  The block's rim is 1 from the outside and the hole's four
    neighbours 1 from the hole; the four diagonal neighbours of the hole are 2 from both, all at squared distance 2 from the
    mean, and the first of them in row-major order wins."""
    lab = shapes.build((9, 9), [["+", "rect", 2, 7, 2, 7], ["-", "rect", 4, 5, 4, 5]])
    got = ref.click(np.zeros_like(lab), lab)
    assert got["fallback"] and got["cand"] == (4, 4) and got["click"] == (3, 3) and got["kind"] == 0
    # 9 x 9 with its centre (5, 5) missing: distance min(to the outside, |dy| + |dx| to the hole) peaks at 3, nearest to the
    # mean at squared distance 5 -- (3, 4) is the first of those eight pixels
    wide = shapes.build((11, 11), [["+", "rect", 1, 10, 1, 10], ["-", "rect", 5, 6, 5, 6]])
    got = ref.click(wide, np.zeros_like(wide))
    assert got["fallback"] and got["cand"] == (5, 5) and got["click"] == (3, 4) and got["kind"] == 1
    assert ref.round_half_even_div(9, 2) == 4 and ref.round_half_even_div(11, 2) == 6 and ref.round_half_even_div(7, 3) == 2


def _argv(argv):
    return ["Tumor" if a == "NF" else a for a in argv] + ["--lits_root", "data/LiTS"]


def test_every_main_eval_line_of_the_shipped_scripts_parses():
    assert len(EVAL_LINES) == 42
    refused = {}
    for script, argv in EVAL_LINES:
        args = main_eval.get_arguments(_argv(argv))
        assert args.tag == os.path.basename(script)[:-3] and args.mode == "eval" and args.lits_root == "data/LiTS"
        assert (args.inter_thresh, args.max_iter, args.infer_set, args.save_path, args.save_subdir) == (0.9, 20, "eval", "prediction", "prediction")
        assert not args.eval_final and args.ckpt_path is None and not args.test and args.seed == 1234
        try:
            assert main_eval.check_args(args) == 2                 # --classes Tumor: stored label >= 2
        except NotImplementedError as e:
            refused[script] = str(e)
    assert sorted(refused) == ["scripts/101_unetinter_v13.sh", "scripts/101_unetinter_v18.sh"]
    assert "--geodesic" in refused["scripts/101_unetinter_v13.sh"] and "--downsampling" in refused["scripts/101_unetinter_v18.sh"]


@pytest.mark.parametrize("flag,name", [("--geodesic", "--geodesic"), ("--fp_sample", "--fp_sample"), ("--sample_neg 0.2", "--sample_neg"),
                                       ("-ds", "--downsampling"), ("--use_context", "--use_context"), ("--test", "--test"),
                                       ("--save_predict", "--save_predict")])
def test_unbuilt_flags_are_refused_by_name_before_anything_is_loaded(flag, name, tmp_path):
    argv = ("--mode eval --tag t --model UNetInter --classes Tumor --im_height 32 --im_width 32 --use_spatial --lits_root {} "
            "--model_dir {}").format(tmp_path / "nowhere", tmp_path / "run").split() + flag.split()
    args = main_eval.get_arguments(argv)
    with pytest.raises(NotImplementedError, match=name):
        main_eval.run(args)                                        # no dataset, no checkpoint, no device: none is reached
    assert not (tmp_path / "run").exists()


def test_max_iter_beyond_the_device_lists_and_bad_sets_are_value_errors():
    base = "--mode eval --tag t --model UNetInter --classes Tumor --im_height 32 --im_width 32 --use_spatial".split()
    with pytest.raises(ValueError, match="--max_iter"):
        main_eval.check_args(main_eval.get_arguments(base + ["--max_iter", "65"]))
    with pytest.raises(ValueError, match="--infer_set"):
        main_eval.check_args(main_eval.get_arguments(base + ["--infer_set", "test"]))
    assert main_eval.check_args(main_eval.get_arguments(base + ["--max_iter", "64", "--infer_set", "train"])) == 2


@pytest.mark.parametrize("rf,plan", [(0, [0]), (1, [0, 1, 3]), (2, [0, 2, 3]), (3, [0, 1, 2, 3])])
def test_mirror_plan_is_run_tta(rf, plan):
    base = "--mode eval --tag t --model UNetInter --classes Tumor --im_height 32 --im_width 32".split()
    args = main_eval.get_arguments(base + ["--random_flip", str(rf), "--eval_mirror"])
    assert main_eval.mirror_plan(args) == plan                    # --random_flip 1 also runs the double flip
    assert main_eval.mirror_plan(main_eval.get_arguments(base + ["--random_flip", str(rf)])) == [0]


def test_dice_is_compute_dice():
    assert main_eval.dice(0, 0, 0) == 1.0 and main_eval.dice(10, 10, 10) == (20 + 1e-8) / (20 + 1e-8)
    assert main_eval.dice(3, 5, 2) == ref.dice(3, 5, 2) == (4 + 1e-8) / (8 + 1e-8)


def test_liver_inter_check_args_is_unchanged_by_the_split():
    import argparse

    from boxsegliver_amd.data import lits_inter
    ok = argparse.Namespace(classes=["Tumor"], mode="train", im_channel=3, guide_channel=2)
    assert lits_inter.check_args(ok) == 2
    with pytest.raises(NotImplementedError, match="offline evaluator"):
        lits_inter.check_args(argparse.Namespace(classes=["Tumor"], mode="eval", im_channel=3))
    with pytest.raises(NotImplementedError, match="--geodesic"):       # the flags come before the mode
        lits_inter.check_args(argparse.Namespace(classes=["Tumor"], mode="eval", geodesic=True))
