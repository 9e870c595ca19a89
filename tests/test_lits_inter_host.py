"""CPU: the `liver_inter` sub-command (data/lits_inter.py) -- flags, refusals, the sampler's split and the click draws --, the
restatement of the click simulator against a brute-force erosion, and the argument checks of the new entry points."""
import ctypes
import json
import os

import numpy as np
import pytest

import lits_inter_ref as ref
from boxsegliver_amd import _abi
from boxsegliver_amd.data import lits3d, lits_inter
from boxsegliver_amd.entry import main as entry

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_run_scripts.json")) as _f:
    RUN_SCRIPTS = json.load(_f)["scripts"]


def _script_argv(extra=()):
    """scripts/101_unetinter_v10.sh's `nf_inter` training line on LiTS: the sub-command, the class and its metric change."""
    (which, argv), = [c for c in RUN_SCRIPTS["scripts/101_unetinter_v10.sh"] if c[0] == "main_g" and "train" in c[1]]
    assert argv[0] == "nf_inter"
    argv = ["liver_inter"] + [{"NF": "Tumor", "NF/Dice": "Tumor/Dice"}.get(a, a) for a in argv[1:]]
    return argv + ["--lits_root", "/data/LiTS"] + list(extra)


@pytest.mark.parametrize("guided", [False, True])
def test_liver_inter_parses_the_reference_script_line(guided):
    args, sub, pipe = entry.get_arguments(_script_argv(), guided=guided)
    assert sub == "liver_inter" and pipe[1] is lits_inter.input_fn
    assert args.model == "UNetInter" and args.classes == ["Tumor"] and args.use_spatial and args.local_enhance
    assert args.stddev == 5.0 and args.guide_channel == 2 and tuple(args.zoom_scale) == (1.0, 1.25) and args.random_flip == 3
    assert args.noise_scale == 0 and args.tumor_percent == 0.5 and args.lits_root == "/data/LiTS" and args.seed == 1234
    assert lits_inter.check_args(args) == 2
    # the flag group is nf_inter's, verbatim
    nf = entry.get_arguments(["nf_inter"] + _script_argv()[1:-2], guided=guided)[0]
    from boxsegliver_amd.data import flagsets
    assert flagsets.PIPELINES["liver_inter"] == flagsets.PIPELINES["nf_g_simply"]
    for flag in flagsets.PIPELINES["nf_g_simply"][0]:
        assert getattr(nf, flag.lstrip("-")) == getattr(args, flag.lstrip("-")), flag


@pytest.mark.parametrize("extra,name", [(["--geodesic"], "--geodesic"), (["--fp_sample"], "--fp_sample"),
                                        (["--sample_neg", "0.25"], "--sample_neg"), (["-ds"], "--downsampling"),
                                        (["--use_context"], "--use_context")])
def test_refused_flags_raise_and_name_themselves(extra, name):
    args, _, _ = entry.get_arguments(_script_argv(extra), guided=True)
    with pytest.raises(NotImplementedError, match=name):
        lits_inter.check_args(args)
    with pytest.raises(NotImplementedError, match=name):
        entry.run(args, "liver_inter", (None, None, None, None), guided=True)       # before anything is loaded


@pytest.mark.parametrize("mode", ["eval", "infer"])
def test_offline_modes_raise(mode):
    argv = _script_argv()
    argv[argv.index("--mode") + 1] = mode
    args, _, _ = entry.get_arguments(argv, guided=True)
    with pytest.raises(NotImplementedError, match="offline evaluator"):
        lits_inter.check_args(args)
    with pytest.raises(NotImplementedError, match="--mode {}".format(mode)):
        entry.run(args, "liver_inter", (None, None, None, None), guided=True)


def test_classes_and_channels():
    args, _, _ = entry.get_arguments(_script_argv(), guided=True)
    assert lits_inter.object_label(["Liver"]) == 1 and lits_inter.object_label(["Tumor"]) == 2
    for bad in (["Liver", "Tumor"], ["NF"], []):
        args.classes = bad
        with pytest.raises(ValueError, match="--classes Liver or --classes Tumor"):
            lits_inter.check_args(args)
    args.classes = ["Liver"]
    for c in (2, 0, 9):
        args.im_channel = c
        with pytest.raises(ValueError, match="--im_channel"):
            lits_inter.check_args(args)
    args.im_channel, args.guide_channel = 1, 3
    with pytest.raises(ValueError, match="--guide_channel"):
        lits_inter.check_args(args)


def test_sampler_split_and_click_draw_ranges():
    """PatchSampler with shape (C, H, W): ceil(bs * tumor_percent) forced samples from the cases with the object, the rest from
    the others; the click draws stay in the ranges `unetk_lits_clicks` takes."""
    depths = (12, 9, 5, 9, 7, 6)
    cases = [{"PID": p, "size": [d, 40, 48]} for p, d in enumerate(depths)]
    offset = {p: int(sum(depths[:p])) for p in range(len(depths))}
    counts = np.zeros(sum(depths), np.int64)
    counts[offset[0] + 3], counts[offset[2] + 1], counts[offset[5] + 2] = 5, 1, 30            # cases 0, 2, 5 hold the object
    s = lits3d.PatchSampler(cases, offset, counts, 5, (3, 32, 32), (40, 48), tumor_percent=0.5, zoom_scale=(1.0, 1.25),
                            random_flip=3, training=True, seed=7)
    for _ in range(50):
        b = s.draw()
        assert b["forced"].tolist() == [True] * 3 + [False] * 2
        assert sorted(b["case"][:3].tolist()) == [0, 2, 5] and set(b["case"][3:].tolist()) <= {1, 3, 4}
        z = b["center"][:3, 0] + np.array([offset[c] for c in b["case"][:3]])
        assert np.all(counts[z] > b["k"][:3])                                               # a rank inside its slice's count
        assert np.all((b["crop"] >= 32) & (b["crop"] <= 40)) and not b["flips"][:, 2].any()
        tab = s.table(b)
        assert tab.shape == (5, _abi.LITS3D_TAB_COLS) and tab.dtype == np.int32
    rng = np.random.default_rng(3)
    t = np.concatenate([lits_inter.draw_click_tab(rng, 64) for _ in range(20)])
    assert t.dtype == np.uint32 and t.shape[1] == _abi.LITS_CLICK_TAB_COLS == ref.CLICK_TAB_COLS
    assert set(t[:, 0].tolist()) == {1, 2, 3, 4} and set(t[:, 1].tolist()) == {0, 1, 2, 3, 4} and set(t[:, 2].tolist()) == {1, 3}
    assert not t[:, 3].any() and t[:, 4:].max() > 1 << 31 and len(np.unique(t[:, 4:])) > 0.99 * t[:, 4:].size
    assert abs((t[:, 2] == 1).mean() - 0.5) < 0.1
    # evaluation: zoom 1.125, no flips, gamma 1
    e = lits3d.PatchSampler(cases, offset, counts, 4, (3, 32, 32), (40, 48), random_flip=3, training=False, seed=7).draw()
    assert np.all(e["crop"] == 36) and not e["flips"].any() and np.all(e["gamma"] == 1)


def test_restated_candidates_equal_a_brute_force_erosion():
    rng = np.random.default_rng(5)
    masks = [rng.random((13, 17)) < 0.8, np.ones((9, 11), bool), np.zeros((9, 11), bool)]
    blob = np.zeros((20, 16), bool)
    blob[4:15, 0:9] = True                                                                  # touches the left border
    masks.append(blob)
    for mask in masks:
        for margin, band in ((1, 2), (2, 3)):
            fg = ref.erode_brute(mask, margin, 0)
            np.testing.assert_array_equal(ref.candidates(mask, margin, band, False), fg)
            outer = ref.erode_brute(~mask, margin, 1)
            np.testing.assert_array_equal(ref.candidates(~mask, margin, band, True), outer ^ ref.erode_brute(outer, band, 1))


def test_restated_simulation_small_case_and_suppression():
    obj = np.zeros((12, 14), np.uint8)
    obj[5:7, 6:8] = 1                                                                       # erosion by 1 empties a 2 x 2 object
    row = np.array([3, 2, 1, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0, 0], np.uint32)
    tr = {}
    pts, cnt = ref.clicks(obj, row, (1, 3, 5, 5), tr)
    assert tr["fg"]["small"] and cnt[0] == 1 and tuple(pts[0, 0]) == (5, 6)                 # floor of the mean (5.5, 6.5)
    assert cnt[1] == 2 and tr["bg"]["ranks"] == [0, tr["bg"]["counts"][1] - 1]              # ranks 0 and count - 1
    d = pts[1, 1] - pts[1, 0]
    assert int(d @ d) > 9                                                                   # outside the first click's circle
    pts, cnt = ref.clicks(np.zeros_like(obj), row, (1, 3, 5, 5), tr)                        # no object: the centre, once
    assert cnt.tolist() == [0, 1] and tuple(pts[1, 0]) == (5, 6) and tr["bg"]["small"]
    pts, cnt = ref.clicks(np.ones_like(obj), row, (1, 3, 5, 5), tr)                         # all object: no background click
    assert cnt[1] == 0 and cnt[0] == 3 and np.all(pts[1] == -1)


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    lib = _abi.lib()
    one = ctypes.c_void_p(4096)                                                             # never dereferenced: the checks come first

    def desc(**kw):
        base = dict(N=2, H=32, W=32, C=3, n_slices=10, src_h=40, src_w=48, im_scale=64, lab_scale=64, obj_label=1, training=0,
                    seed=0, noise_scale=0.0, margin=3, step=10, band=40, max_clicks=5, G=2, gaussian=0, stddev=3.0)
        base.update(kw)
        return _abi.LitsInterDesc(**base)
    good = desc()
    assert lib.unetk_lits_inter_batch_ws_bytes(ctypes.byref(good)) > 0
    assert lib.unetk_lits_clicks_ws_bytes(ctypes.byref(good)) >= 2 * 3 * 40 * 48
    for bad in (desc(C=2), desc(C=9), desc(H=1 << 15, W=1 << 15)):
        assert lib.unetk_lits_inter_batch_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.unetk_lits_inter_batch(ctypes.byref(bad), one, one, one, one, one, one, one, 1 << 20, None) == -2
    for bad in (desc(margin=0), desc(band=0), desc(margin=200, band=55), desc(max_clicks=6), desc(max_clicks=1), desc(src_w=1025),
                desc(step=-1)):
        assert lib.unetk_lits_clicks_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.unetk_lits_clicks(ctypes.byref(bad), one, one, one, one, one, one, one, 1 << 20, None) == -2
    for bad in (desc(N=0), desc(H=0), desc(obj_label=0), desc(lab_scale=0), desc(n_slices=0)):
        assert lib.unetk_lits_inter_batch_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.unetk_lits_inter_batch(ctypes.byref(bad), one, one, one, one, one, one, one, 1 << 20, None) == -1
        assert lib.unetk_lits_clicks(ctypes.byref(bad), one, one, one, one, one, one, one, 1 << 20, None) == -1
        assert lib.unetk_click_guide(ctypes.byref(bad), one, one, one, one, None) == -1
    args = [one] * 7
    for i in range(7):                                                                      # every NULL pointer
        a = list(args)
        a[i] = None
        assert lib.unetk_lits_inter_batch(ctypes.byref(good), *a, 1 << 20, None) == -1
        assert lib.unetk_lits_clicks(ctypes.byref(good), *a, 1 << 20, None) == -1
    for i in range(4):
        a = [one] * 4
        a[i] = None
        assert lib.unetk_click_guide(ctypes.byref(good), *a, None) == -1
    assert lib.unetk_click_guide(ctypes.byref(desc(G=3)), one, one, one, one, None) == -1
    assert lib.unetk_click_guide(ctypes.byref(desc(gaussian=1, stddev=0.0)), one, one, one, one, None) == -1
    assert lib.unetk_lits_inter_batch(ctypes.byref(good), one, one, one, one, one, one, one, 8, None) == -3     # short workspace
    assert lib.unetk_lits_clicks(ctypes.byref(good), one, one, one, one, one, one, one, 8, None) == -3
    assert lib.unetk_lits_inter_batch(ctypes.byref(good), one, one, one, one, one, one, ctypes.c_void_p(4104), 1 << 20, None) == -1
    assert lib.unetk_lits_inter_batch(ctypes.byref(good), one, one, ctypes.c_void_p(4098), one, one, one, one, 1 << 20, None) == -1
