"""GPU: the spatial guide of the guided LiTS pipeline -- `unetk_lits_spatial_guide` (csrc/lits.hip) against the numpy
restatement of the reference's render (test_lits_guide_host.render_numpy) and against the reference's own renderer
(tests/golden/ref_sp_guide.npz), its buffer edges, its alignment with the image / label kernel, the pipeline's guarantees
(a guided run draws the same batches; eval_3d guides are fixed), and `main_g liver ... --use_spatial` end to end."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from guardbuf import Guarded
from test_lits_guide_host import GOLDEN, render_numpy

pytestmark = pytest.mark.gpu


def _guide(tab, ptr, obj, out_hw, c, src_hw, min_std=1.0):
    from boxsegliver_amd import ops
    return ops.lits_spatial_guide(torch.from_numpy(np.asarray(tab, np.int32)).cuda(),
                                  torch.from_numpy(np.asarray(ptr, np.int32)).cuda(),
                                  torch.from_numpy(np.asarray(obj, np.float32).reshape(-1, 4)).cuda(),
                                  out_hw, c, src_hw, min_std).cpu().numpy()


def _random_batch(rng, n, c, src_hw, counts):
    """A table with zoomed / shrunk, non-square crops inside the slice, random flips, and `counts[j]` objects per sample:
    centres in and around the crop, stddevs from 0 (floored) to wider than the crop."""
    sh, sw = src_hw
    tab = np.zeros((n, c + 7), np.int32)
    objs = []
    for j in range(n):
        ch, cw = int(rng.integers(1, sh + 1)), int(rng.integers(1, sw + 1))
        tab[j, c + 1:c + 5] = [rng.integers(0, sh - ch + 1), rng.integers(0, sw - cw + 1), ch, cw]
        tab[j, c + 5:] = rng.integers(0, 2, 2)
        k = counts[j]
        cen = np.stack([rng.uniform(-4, ch + 4, k), rng.uniform(-4, cw + 4, k)], axis=1)
        sd = rng.choice([0.0, 0.3, 1.0, 2.5, 7.0, 60.0], size=(k, 2))
        objs.append(np.concatenate([cen, sd], axis=1))
    ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return tab, ptr, np.concatenate(objs).astype(np.float32).reshape(-1, 4)


@pytest.mark.parametrize("out_hw", [(32, 32), (24, 40), (17, 9), (1, 1), (1, 13), (31, 1)])
def test_kernel_matches_numpy_restatement(out_hw):
    rng = np.random.default_rng(11 + out_hw[0] * 7 + out_hw[1])
    src_hw, c = (61, 47), 3
    counts = [0, 1, 40, 3, 0, 2, 15, 1]
    tab, ptr, obj = _random_batch(rng, len(counts), c, src_hw, counts)
    got = _guide(tab, ptr, obj, out_hw, c, src_hw)
    want = render_numpy(tab, ptr, obj, out_hw, c, src_hw)
    assert got.shape == (len(counts),) + out_hw + (1,)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    for j, k in enumerate(counts):
        if k == 0:
            assert np.all(got[j] == np.float32(0.5)), j                    # the reference's false_fn, exactly
    assert got[2].max() > 0.5                                            # 40 objects: the guide is not flat


def test_min_std_floor_and_crop_clamp():
    """stddevs below the floor render as the floor; a crop reaching past the slice is clamped like unetk_lits_batch's."""
    c, src_hw = 1, (20, 20)
    obj = np.array([[5.0, 6.0, 0.0, 0.2], [5.0, 6.0, 3.0, 3.0]], np.float32)
    tab = np.array([[0, 0, 2, 3, 12, 10, 0, 0], [0, 0, 2, 3, 12, 10, 0, 0], [0, 0, 15, -4, 30, 50, 1, 1]], np.int32)
    ptr = [0, 1, 2, 3]
    got = _guide(tab, ptr, np.concatenate([obj, obj[:1]]), (16, 16), c, src_hw, min_std=3.0)
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_allclose(got, render_numpy(tab, ptr, np.concatenate([obj, obj[:1]]), (16, 16), c, src_hw, 3.0), atol=2e-6)


def test_kernel_reproduces_the_reference_renderer():
    """crop == output size: the kernel's guide is g / 2 + 0.5 of the reference's create_gaussian_distribution_v2."""
    z = np.load(GOLDEN)
    for i, (h, w, k) in enumerate(z["shapes"].tolist()):
        obj = np.concatenate([z["case{}_centers".format(i)], z["case{}_stddevs".format(i)]], axis=1)
        tab = np.array([[0, 0, 0, 0, h, w, 0, 0]], np.int32)
        got = _guide(tab, [0, k], obj, (h, w), 1, (h, w))
        np.testing.assert_allclose(got[0, ..., 0], z["case{}_guide".format(i)] / np.float32(2) + np.float32(0.5), rtol=0, atol=2e-6,
                                   err_msg="case {}".format(i))


@pytest.mark.parametrize("out_hw,n", [((17, 9), 3), ((1, 1), 5), ((64, 48), 2)])
def test_guard_bands(out_hw, n):
    """Every output element is written, nothing outside the view is touched, the inputs stay bit-equal."""
    from boxsegliver_amd import _abi
    rng = np.random.default_rng(3)
    c, src_hw = 3, (40, 30)
    counts = [0, 4, 1, 0, 2][:n]
    tab, ptr, obj = _random_batch(rng, n, c, src_hw, counts)
    out = Guarded((n,) + out_hw + (1,))
    tab_t, ptr_t, obj_t = (torch.from_numpy(a).cuda() for a in (tab, ptr, obj))
    snaps = [t.clone() for t in (tab_t, ptr_t, obj_t)]
    d = _abi.LitsGuideDesc(n, out_hw[0], out_hw[1], c, src_hw[0], src_hw[1], len(obj), 1.0)
    rc = _abi.lib().unetk_lits_spatial_guide(ctypes.byref(d), ctypes.c_void_p(tab_t.data_ptr()), ctypes.c_void_p(ptr_t.data_ptr()),
                                             ctypes.c_void_p(obj_t.data_ptr()), ctypes.c_void_p(out.ptr()),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert out.unwritten() == 0 and out.check_untouched()
    assert all(torch.equal(a, b) for a, b in zip((tab_t, ptr_t, obj_t), snaps))
    np.testing.assert_allclose(out.view.cpu().numpy(), render_numpy(tab, ptr, obj, out_hw, c, src_hw), atol=2e-6)
    # refusals before any launch: NULL output, a zero floor, a misaligned object table
    for bad in (dict(guide=None), dict(min_std=0.0), dict(obj_off=4)):
        dd = _abi.LitsGuideDesc(n, out_hw[0], out_hw[1], c, src_hw[0], src_hw[1], len(obj), bad.get("min_std", 1.0))
        rc = _abi.lib().unetk_lits_spatial_guide(ctypes.byref(dd), ctypes.c_void_p(tab_t.data_ptr()), ctypes.c_void_p(ptr_t.data_ptr()),
                                                 ctypes.c_void_p(obj_t.data_ptr() + bad.get("obj_off", 0)),
                                                 None if "guide" in bad else ctypes.c_void_p(out.ptr()),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0, bad
    torch.cuda.synchronize()
    assert out.check_untouched()


# ------------------------------------------------------------------------------------------------- the pipeline
def _args(**over):
    a = argparse.Namespace(test_fold=2, filter_size=0, batch_size=8, num_gpus=1, im_height=32, im_width=32, im_channel=3,
                           noise_scale=0.05, zoom_scale=(1.0, 1.25), random_flip=3, seed=77, eval_num_batches_per_epoch=3,
                           eval_3d=False, use_spatial=True, spatial_random=1.0, spatial_inner_random=False,
                           center_random_ratio=0.2, stddev_random_ratio=0.4, min_std=2.0)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _params(root, args):
    return {"args": args, "lits_root": str(root)}


def _take(gen, n):
    return [next(gen) for _ in range(n)]


def test_guide_lines_up_with_the_labels(tmp_path):
    """Exact moments (ratios 0), flips on: wherever a guide is not constant, its peak lies on a tumour pixel of the same
    sample -- a crop or flip mismatch between the guide kernel and the image / label kernel would move it off."""
    from boxsegliver_amd.data import lits
    from test_gpu_lits import _write_dataset
    _write_dataset(tmp_path)
    args = _args(center_random_ratio=0.0, stddev_random_ratio=0.0, noise_scale=0.0)
    peaks = 0
    for feats, labels in _take(lits.input_fn("train", _params(tmp_path, args)), 12):
        g = feats["sp_guide"]
        assert g.shape == (8, 32, 32, 1) and g.dtype == torch.float32 and g.is_cuda
        g, lab = g.cpu().numpy()[..., 0], labels.cpu().numpy()
        for j in range(8):
            if g[j].max() == g[j].min():
                assert g[j].max() == np.float32(0.5)
                continue
            y, x = np.unravel_index(np.argmax(g[j]), g[j].shape)
            assert lab[j, y, x] == 2, (j, y, x)
            peaks += 1
    assert peaks >= 30                                     # forced tumour share: >= 4 tumour slices per batch


def test_guided_run_draws_the_same_batches(tmp_path):
    from boxsegliver_amd.data import lits
    from test_gpu_lits import _write_dataset
    _write_dataset(tmp_path)
    guided = _take(lits.input_fn("train", _params(tmp_path, _args())), 4)
    plain = _take(lits.input_fn("train", _params(tmp_path, _args(use_spatial=False, liver_percent=0.66, tumor_percent=0.5))), 4)
    for (fg, lg), (fp, lp) in zip(guided, plain):
        assert "sp_guide" not in fp
        assert torch.equal(fg["images"], fp["images"]) and torch.equal(lg, lp) and torch.equal(fg["names"], fp["names"])
    assert any(float(f["sp_guide"].max()) > 0.75 for f, _ in guided)
    # the guided pipeline's forced shares are the reference's constants, whatever the unguided flags say
    again = _take(lits.input_fn("train", _params(tmp_path, _args(liver_percent=0.0, tumor_percent=0.0))), 4)
    for (fg, lg), (fa, la) in zip(guided, again):
        assert torch.equal(fg["images"], fa["images"]) and torch.equal(fg["sp_guide"], fa["sp_guide"])
    with pytest.raises(ValueError):
        lits.input_fn("train", _params(tmp_path, _args(guide_channel=2)))


def test_spatial_random_zero_and_eval_online(tmp_path):
    from boxsegliver_amd.data import lits
    from test_gpu_lits import _write_dataset
    _write_dataset(tmp_path)
    for feats, _ in _take(lits.input_fn("train", _params(tmp_path, _args(spatial_random=0.0))), 3):
        assert bool((feats["sp_guide"] == 0.5).all())
    # eval_online 2-D: spatial_random < 1 -> no guide at all; = 1 -> guides on the tumour slices
    ev = list(lits.input_fn("eval_online", _params(tmp_path, _args(spatial_random=0.9))))
    assert len(ev) == 3 and all(bool((f["sp_guide"] == 0.5).all()) for f, _ in ev)
    ev = list(lits.input_fn("eval_online", _params(tmp_path, _args())))
    assert len(ev) == 3 and any(float(f["sp_guide"].max()) > 0.75 for f, _ in ev)


def test_eval_3d_guides_are_fixed(tmp_path):
    from boxsegliver_amd.data import lits
    from test_gpu_lits import _write_dataset
    _write_dataset(tmp_path, n_cases=4, depth=7)
    (tmp_path / "k_folds.txt").write_text("Fold 0:0 1\nFold 1:2 3\n")
    args = _args(eval_3d=True, test_fold=1, batch_size=4)
    params = _params(tmp_path, args)
    one = list(lits.input_fn("eval_online", params))
    two = list(lits.input_fn("eval_online", params))
    # 2 cases x liver z range [1, 6) = 5 slices -> 2 batches of 4 each; slices 1..5 -> batch rows; 3 padding rows at the end
    assert len(one) == len(two) == 4
    for (f1, l1), (f2, l2) in zip(one, two):
        assert torch.equal(f1["sp_guide"], f2["sp_guide"]) and torch.equal(f1["images"], f2["images"])
    for k in (0, 2):
        g = torch.cat([one[k][0]["sp_guide"], one[k + 1][0]["sp_guide"]]).cpu().numpy()[..., 0]
        lab = torch.cat([one[k][1], one[k + 1][1]]).cpu().numpy()
        assert np.all(g[5:] == np.float32(0.5))                                  # padding slices
        for s, z in enumerate(range(1, 6)):
            if z in (2, 3):                                                     # the tumour slices
                y, x = np.unravel_index(np.argmax(g[s]), g[s].shape)
                assert g[s].max() > 0.9 and lab[s, y, x] == 2
            else:
                assert np.all(g[s] == np.float32(0.5))


@pytest.mark.parametrize("eval_3d", [False, True])
def test_main_g_liver_trains_with_the_spatial_guide_end_to_end(tmp_path, eval_3d):
    """`main_g liver --model GUNet --model_config GUNet_SP.yml --use_spatial --spatial_random 1.0 ...` (the reference's
    run_scripts/template/002_gnet_sp.sh) on the synthetic on-disk dataset: trains, evaluates online, keeps the best."""
    from boxsegliver_amd.entry import main_g
    from test_gpu_lits import _write_dataset
    _write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = ("liver --mode train --tag gsp --model GUNet --model_config GUNet_SP.yml --classes Liver Tumor --test_fold 2 "
            "--im_height 32 --im_width 32 --im_channel 3 --noise_scale 0.05 --zoom_scale 1.0 1.25 --random_flip 3 --num_of_steps 4 "
            "--primary_metric Tumor/Dice --secondary_metric Liver/Dice --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--batches_per_epoch 2 --batch_size 4 --weight_decay_rate 0.000001 --learning_policy plateau --learning_rate 0.001 "
            "--lr_end 0 --lr_decay_rate 0.2 --normalizer instance_norm --use_spatial --spatial_random 1.0 "
            "--eval_num_batches_per_epoch 2 --eval_per_epoch --evaluator Volume --save_best --log_step 1").split()
    argv += ["--lits_root", str(tmp_path), "--model_dir", str(run)] + (["--eval_3d"] if eval_3d else [])
    assert main_g.main(argv) == 0
    assert json.load(open(str(run / "checkpoint")))["global_step"] == 4
    assert os.path.exists(str(run / "checkpoint_best")) and os.path.exists(str(run / "best_result"))
    best = json.load(open(str(run / "best_result")))
    assert "Tumor/Dice" in best.get("ma_results", best)
