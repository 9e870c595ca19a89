"""CPU: the `liver_3d` sub-command (UNet3D on LiTS, data/lits3d.py) -- flag parsing, the patch sampler's policy
(DataLoader/NF/input_pipeline_3d.py:544-604 gen_batch) and the invariants of the float64 restatement the GPU tests of
`unetk_lits_patch3d` lean on (lits3d_ref.py)."""
import math

import numpy as np
import pytest

import lits3d_ref as ref

# threed_script/201_unet_v1.sh's flag list with the sub-command and the classes changed
SCRIPT_3D = ("liver_3d --mode train --tag 201_unet_v1 --model UNet3D --classes Liver Tumor --test_fold 2 --im_depth 10 --im_height 256 "
             "--im_width 256 --im_channel 1 --random_flip 7 --num_of_total_steps 400000 --primary_metric Tumor/Dice "
             "--loss_weight_type numerical --loss_numeric_w 1 1 3 --batches_per_epoch 2000 --batch_size 4 --weight_decay_rate 0.00003 "
             "--learning_policy plateau --learning_rate 0.0003 --lr_end 0.0000005 --lr_decay_rate 0.2 --lr_patience 30 "
             "--eval_num_batches_per_epoch 200 --eval_per_epoch --evaluator Volume --normalizer instance_norm --tumor_percent 0.75 "
             "--save_best --summary_prefix liver --log_step 125 --lits_root /data/LiTS").split()


def _sampler(bs=4, tumor_percent=0.75, training=True, seed=7, shape=(6, 16, 20), fg=2, **kw):
    from boxsegliver_amd.data import lits3d
    cases = ref.make_cases()
    _, lb, base = ref.stack_store(cases)
    counts = (lb // 64 >= fg).sum(axis=(1, 2))
    meta = [{"PID": pid, "size": [im.shape[0], ref.H, ref.W]} for pid, (im, _) in enumerate(cases)]
    offset = {pid: int(b) for pid, b in enumerate(base)}
    return lits3d.PatchSampler(meta, offset, counts, bs, shape, (ref.H, ref.W), tumor_percent=tumor_percent, training=training,
                               seed=seed, **kw), cases, base


def test_liver_3d_parses_the_reference_3d_script_flags():
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    args, sub, pipe = entry.get_arguments(SCRIPT_3D)
    assert sub == "liver_3d" and pipe[1] is lits3d.input_fn and pipe[2] is lits3d.input_fn_eval
    assert (args.im_depth, args.im_height, args.im_width, args.im_channel) == (10, 256, 256, 1)
    assert args.random_flip == 7 and args.tumor_percent == 0.75 and args.batch_size == 4 and args.classes == ["Liver", "Tumor"]
    assert args.eval_num_batches_per_epoch == 200 and args.lits_root == "/data/LiTS" and args.seed == 1234
    # the reference's defaults (input_pipeline_3d.py:53-67)
    d, _, _ = entry.get_arguments("liver_3d --mode train --tag t --model UNet3D --classes Liver".split())
    assert (d.test_fold, d.im_depth, d.im_height, d.im_width, d.im_channel) == (2, 10, 256, 256, 1)
    assert tuple(d.zoom_scale) == (1.0, 1.25) and d.random_flip == 1 and d.eval_num_batches_per_epoch == 100
    assert d.tumor_percent == 0.5
    assert lits3d.check_args(args) == (2, 2) and lits3d.check_args(d) == (1, 1)          # (lab_max, fg_label)
    bad, _, _ = entry.get_arguments("liver_3d --mode train --tag t --model UNet3D --classes Liver --im_channel 3".split())
    with pytest.raises(ValueError, match="one channel"):
        lits3d.check_args(bad)
    with pytest.raises(ValueError, match="--classes"):
        lits3d.label_map(["Tumor"])
    with pytest.raises(ValueError):
        entry.get_arguments(SCRIPT_3D, guided=True)                                          # not a main_g sub-command
    with pytest.raises(NotImplementedError, match="whole-volume 3-D evaluation"):
        lits3d.input_fn_eval("eval", {"args": args})
    with pytest.raises(ValueError, match="train"):
        lits3d.input_fn("eval", {"args": args})


@pytest.mark.parametrize("bs,tp", [(4, 0.75), (3, 0.5), (2, 0.0), (3, 1.0)])
def test_sampler_forced_share_and_remainder(bs, tp):
    s, cases, base = _sampler(bs=bs, tumor_percent=tp)
    force = int(math.ceil(bs * tp))
    tumour_cases = {0, 2, 3}
    for _ in range(40):
        b = s.draw()
        assert b["forced"].sum() == force and b["forced"][:force].all()
        assert set(b["case"][:force].tolist()) <= tumour_cases                       # forced: cases that hold the class
        assert len(set(b["case"].tolist())) == bs                                     # both draws without replacement, disjoint
        tab = s.table(b)
        assert tab.dtype == np.int32 and tab.shape == (bs, 16)
        np.testing.assert_array_equal(tab[:, 0], base[b["case"]])
        np.testing.assert_array_equal(tab[:, 1], np.array(ref.DEPTHS)[b["case"]])
        np.testing.assert_array_equal(tab[:, 10].view(np.float32), b["gamma"])
        for j in range(bs):
            im, lab = cases[b["case"][j]]
            z = b["center"][j, 0]
            assert 0 <= z < im.shape[0]
            if b["forced"][j]:
                assert 0 <= b["k"][j] < (lab[z] == 2).sum()                           # a rank inside the slice's count
            else:
                assert 0 <= b["center"][j, 1] < ref.H and 0 <= b["center"][j, 2] < ref.W
        assert np.all((b["gamma"] >= 0.7) & (b["gamma"] <= 1.5))


def test_rank_to_slice_and_in_slice_rank_match_brute_force():
    for fg in (1, 2):
        s, cases, _ = _sampler(fg=fg)
        for ci, (_, lab) in enumerate(cases):
            pos = np.argwhere(lab >= fg)                                              # the reference's data[pid]['pos'], z-major
            assert len(pos) == s.case_total[ci]
            if len(pos) == 0:
                continue
            ranks = np.arange(len(pos))
            z, k = s.locate(np.full(len(pos), ci), ranks)
            np.testing.assert_array_equal(z, pos[:, 0])
            for r in (0, len(pos) - 1, len(pos) // 2):
                in_slice = np.argwhere(lab[z[r]] >= fg)
                np.testing.assert_array_equal(in_slice[k[r]], pos[r, 1:])
    # the single-pixel slice is reachable and has rank 0
    s, cases, _ = _sampler()
    pos = np.argwhere(cases[0][1] >= 2)
    r = int(np.flatnonzero((pos == np.array(ref.SINGLE_PIXEL)).all(axis=1))[0])
    z, k = s.locate([0], [r])
    assert (int(z[0]), int(k[0])) == (ref.SINGLE_PIXEL[0], 0)
    # every forced-class voxel is drawn about equally often
    s, cases, _ = _sampler(bs=1, tumor_percent=1.0, seed=3)
    hits = {}
    for _ in range(3000):
        b = s.draw()
        key = (int(b["case"][0]), int(b["center"][0, 0]))
        hits[key] = hits.get(key, 0) + 1
    for (ci, z), n in hits.items():
        share = (cases[ci][1][z] == 2).sum() / (cases[ci][1] == 2).sum() / 3.0          # 3 tumour cases, uniform
        assert abs(n / 3000.0 - share) < 0.03, (ci, z, n)


def test_crop_shapes_truncate_as_astype_int32():
    from boxsegliver_amd.data import lits3d
    target = np.array([10, 256, 256], dtype=np.float32)
    rng = np.random.default_rng(0)
    for _ in range(200):
        zoom = rng.uniform(1.0, 1.25, size=2).tolist()
        want = (target * ([1] + zoom)).astype(np.int32)                                # input_pipeline_3d.py:589, verbatim
        np.testing.assert_array_equal(lits3d.crop_shape([256, 256], zoom), want[1:])
    np.testing.assert_array_equal(lits3d.crop_shape([256, 256], [1.125, 1.125]), [288, 288])
    np.testing.assert_array_equal(lits3d.crop_shape([16, 20], [1.4, 1.4]), [22, 28])       # 22.4 -> 22: truncation, not rounding
    s, _, _ = _sampler(zoom_scale=(1.0, 1.4))
    b = s.draw()
    assert b["crop"].dtype == np.int32 and np.all(b["crop"] >= [16, 20]) and np.all(b["crop"] <= [22, 28])


def test_eval_stream_repeats_and_training_streams_differ_per_rank():
    def stream(**kw):
        s, _, _ = _sampler(**kw)
        return np.stack([s.table() for _ in range(5)])
    np.testing.assert_array_equal(stream(training=False, seed=1234 + 500), stream(training=False, seed=1234 + 500))
    ev = stream(training=False, seed=1234 + 500, random_flip=7)
    assert np.all(ev[:, :, 5:7] == [18, 22])                                          # zoom fixed at 1.125
    assert np.all(ev[:, :, 7:10] == 0) and np.all(ev[:, :, 10].view(np.float32) == 1.0)   # no flips, no gamma
    r0, r1 = stream(seed=1234, random_flip=7), stream(seed=1234 + 1000, random_flip=7)
    assert not np.array_equal(r0, r1)
    np.testing.assert_array_equal(r0, stream(seed=1234, random_flip=7))
    assert r0[:, :, 7:10].any() and r0[:, :, 9].any()                                  # the front/back bit flips slices
    assert not stream(seed=1234, random_flip=3)[:, :, 9].any()                         # only the enabled axes


def test_too_few_cases_raise():
    with pytest.raises(ValueError, match="too few cases with forced-class voxels"):
        _sampler(bs=4, tumor_percent=1.0)                                             # 4 forced, 3 tumour cases
    with pytest.raises(ValueError, match="too few cases"):
        _sampler(bs=6, tumor_percent=0.5)                                             # 3 forced + 3 others, 1 other case left


def test_restatement_zscore_invariants():
    cases = ref.make_cases()
    im, lab = cases[0]
    box = ref.crop_box((6, 20, 40), (22, 28), (6, 16, 20), im.shape[0], (ref.H, ref.W))
    img, _ = ref.crop(im, lab, box, 6)
    z, m, s = ref.zscore(img)
    mask = img > 0
    assert mask.any() and not mask.all()
    assert abs(z[mask].mean()) < 1e-12 and abs(z[mask].std() - 1.0) < 1e-7              # masked mean 0, std 1 (1e-8 epsilon)
    assert np.all(z[~mask] == 0)
    # a crop at a corner stays inside the volume; a shallow case starts at 0 and is zero-padded
    assert ref.crop_box((0, 0, 0), (22, 28), (6, 16, 20), 12, (ref.H, ref.W)) == (0, 0, 0, 22, 28)
    assert ref.crop_box((11, 39, 47), (22, 28), (6, 16, 20), 12, (ref.H, ref.W)) == (6, 18, 20, 22, 28)
    assert ref.crop_box((4, 20, 20), (50, 60), (6, 16, 20), 5, (ref.H, ref.W)) == (0, 0, 0, 40, 48)
    img, lb = ref.crop(cases[2][0], cases[2][1], (0, 0, 0, 40, 48), 6)
    assert np.all(img[5] == 0) and np.all(lb[5] == 0) and img[4].any()
    # empty and constant masks: finite, all zeros
    for region in (ref.AIR, ref.FLAT):
        img = cases[1][0][(slice(0, 6),) + region].astype(np.float64) / 64
        z, m, s = ref.zscore(img)
        assert s == 0 and np.all(z == 0)


def test_restatement_gamma_retains_the_statistics():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 16, 20))
    x = (x - x.mean()) / x.std()                                                       # a z-scored patch: mean 0, std 1
    for gamma in (0.7, 0.93, 1.0, 1.5):
        y = ref.augment_gamma(x, gamma)
        assert abs(y.mean() - x.mean()) < 1e-12 and abs(y.std() - x.std()) < 1e-7      # mean kept; std to the 1e-8 epsilon
    # the literal formula rescales AFTER re-centring: a patch with mean mn != 0 comes out with mean mn * sd / (new_sd + 1e-8)
    x2 = x * 2.0 + 0.5
    y2 = ref.augment_gamma(x2, 0.8)
    mapped = np.power((x2 - x2.min()) / (x2.max() - x2.min() + 1e-7), 0.8) * (x2.max() - x2.min()) + x2.min()
    assert abs(y2.mean() - 0.5 * x2.std() / (mapped.std() + 1e-8)) < 1e-12 and abs(y2.std() - x2.std()) < 1e-7
    for const in (0.0, 3.0):                                                           # a constant patch: finite, zero
        y = ref.augment_gamma(np.full((2, 4, 4), const), 0.8)
        assert np.all(np.isfinite(y)) and np.all(y == 0)


def test_abi_argument_validation_without_gpu():
    """Every refusal of the two entry points returns before anything is launched."""
    import ctypes
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    d = _abi.Lits3dDesc(4, 10, 256, 256, 1000, 512, 512, 64, 64, 2, 1)
    nbytes = lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(d))
    assert nbytes == 4 * 160 * 32 + 4 * 32                      # 160 partial blocks of {3 doubles, 2 floats} + 8 floats, per sample
    p = ctypes.c_void_p(1 << 20)                                # never dereferenced: the calls below return first
    assert lib.unetk_lits_patch3d(ctypes.byref(d), p, p, p, p, p, p, nbytes - 1, None) == -3            # UNETK_E_WORKSPACE
    assert lib.unetk_lits_patch3d(ctypes.byref(d), p, p, p, p, None, p, nbytes, None) == -1             # UNETK_E_BADARG
    assert lib.unetk_lits_patch3d(ctypes.byref(d), p, p, p, p, p, ctypes.c_void_p((1 << 20) + 8), nbytes, None) == -1
    assert lib.unetk_lits_patch3d(ctypes.byref(d), p, p, p, ctypes.c_void_p((1 << 20) + 2), p, p, nbytes, None) == -1
    big = _abi.Lits3dDesc(1, 2048, 1024, 1024, 1000, 512, 512, 64, 64, 2, 0)                            # D*H*W = 2^31
    assert lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(big)) == 0
    assert lib.unetk_lits_patch3d(ctypes.byref(big), p, p, p, p, p, p, 1 << 30, None) == -2             # UNETK_E_UNSUPPORTED
    deep = _abi.Lits3dDesc(1, 8192, 96, 96, 10000, 512, 512, 64, 64, 2, 0)                              # D*src_h*src_w = 2^31
    assert lib.unetk_lits_patch3d(ctypes.byref(deep), p, p, p, p, p, p, 1 << 30, None) == -2
    for bad in (_abi.Lits3dDesc(0, 10, 256, 256, 1000, 512, 512, 64, 64, 2, 1), _abi.Lits3dDesc(4, 10, 256, 256, 1000, 512, 512, 64, 0, 2, 1)):
        assert lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.unetk_lits_patch3d(ctypes.byref(bad), p, p, p, p, p, p, 1 << 30, None) == -1
    assert lib.unetk_lits_pick_voxel(None, 10, 40, 48, 64, 2, p, 2, p, None) == -1
    assert lib.unetk_lits_pick_voxel(p, 10, 40, 48, 64, 0, p, 2, p, None) == -1                         # fg_label < 1
    assert lib.unetk_lits_pick_voxel(p, 10, 40, 48, 64, 2, p, 0, p, None) == -1
