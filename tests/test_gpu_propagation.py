"""GPU: the spatial-guide propagation of the guided volume evaluation -- `unetk_guide_components` (csrc/evalvol.hip) and
`unetk_guide_render` (csrc/lits.hip) against their numpy restatements (data/propagate.py), their buffer edges and
repeatability, the device-driven loop of EvaluateVolume.run_g against a host-driven one, and `main_g liver --mode eval
--use_spatial` end to end (with and without the context guide, and with --eval_no_sp)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from guardbuf import Guarded, GuardedWorkspace, guarded_input

pytestmark = pytest.mark.gpu


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _acc_of(mask, rng, ties=True):
    """Probabilities whose argmax == 2 is exactly `mask`; where `ties`, some background pixels tie classes 1 and 2 (the
    first index wins, so they stay background)."""
    h, w = mask.shape
    acc = rng.random((h, w, 3)).astype(np.float32) * 0.3
    acc[..., 0] = np.where(mask, acc[..., 0], np.float32(0.6))
    acc[..., 2] = np.where(mask, np.float32(0.9), acc[..., 2])
    if ties:
        tie = (~mask) & (rng.random((h, w)) < 0.05)
        acc[..., 1] = np.where(tie, np.float32(0.95), acc[..., 1])
        acc[..., 2] = np.where(tie, np.float32(0.95), acc[..., 2])
    return acc


def _random_mask(rng, shape, density, blobs=0):
    mask = rng.random(shape) < density
    for _ in range(blobs):
        y, x = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        mask[y:y + rng.integers(1, 30), x:x + rng.integers(1, 30)] = True
    mask[0, :] |= rng.random(shape[1]) < 0.5                        # the image border
    mask[:, -1] |= rng.random(shape[0]) < 0.5
    return mask


def _check(mask, guide, acc=None, cap=32768):
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import propagate
    rng = np.random.default_rng(0)
    acc = _acc_of(mask, rng) if acc is None else acc
    table = ops.guide_components(torch.from_numpy(acc).cuda(), torch.from_numpy(guide).cuda(), cap).cpu().numpy()
    got, _ = propagate.parse_table(table, mask.shape[1])
    want = propagate.components_numpy(np.argmax(acc, -1) == 2, guide)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.root, g.area, g.box, g.peak) == (w.root, w.area, w.box, w.peak)
        assert g.peak_value == w.peak_value
        np.testing.assert_array_equal(g.center, w.center)
        np.testing.assert_array_equal(g.stddev, w.stddev)
    return got


@pytest.mark.parametrize("shape,density,blobs", [((256, 256), 0.3, 0), ((256, 256), 0.02, 60), ((512, 512), 0.1, 0),
                                                 ((512, 512), 0.01, 200), ((97, 131), 0.5, 5)])
def test_components_match_the_restatement(shape, density, blobs):
    rng = np.random.default_rng(hash((shape, density)) % 1000)
    mask = _random_mask(rng, shape, density, blobs)
    guide = (rng.integers(0, 8, shape) / 8.).astype(np.float32) + np.float32(0.5)    # few levels: ties on the peak
    got = _check(mask, guide)
    assert len(got) > 100 or blobs
    areas = np.array([c.area for c in got])
    assert (areas == 1).any() and (areas % 2 == 0).any() and (areas % 2 == 1).any()
    assert any(c.center[0] % 1 == 0.5 for c in got)                  # .5 medians


def test_components_single_pixels_borders_and_empty():
    rng = np.random.default_rng(1)
    mask = np.zeros((64, 80), bool)
    mask[::2, ::2] = True                                            # hundreds of single pixels, corners and edges included
    guide = rng.random((64, 80)).astype(np.float32)
    got = _check(mask, guide)
    assert len(got) == mask.sum()
    assert not _check(np.zeros((64, 80), bool), guide)
    full = _check(np.ones((64, 80), bool), guide)
    assert len(full) == 1 and full[0].box == (0, 0, 63, 79)


def test_components_overflow_flag():
    from boxsegliver_amd import ops
    mask = np.zeros((32, 32), bool)
    mask[::2, ::2] = True
    acc = _acc_of(mask, np.random.default_rng(2), ties=False)
    t = ops.guide_components(torch.from_numpy(acc).cuda(), torch.full((32, 32), 0.5, device="cuda"), 100).cpu().numpy()
    assert t[0] == 256 and t[1] == 1


def test_components_guard_bands_and_repeatability():
    from boxsegliver_amd import _abi
    rng = np.random.default_rng(4)
    h, w, cap = 120, 136, 700
    mask = _random_mask(rng, (h, w), 0.03)                          # about 530 components: rows left unwritten
    acc = guarded_input(torch.from_numpy(_acc_of(mask, rng)).cuda())
    guide = guarded_input(torch.from_numpy(rng.random((h, w, 1)).astype(np.float32)).cuda())
    lib = _abi.lib()
    nbytes = lib.unetk_guide_components_ws_bytes(h, w, cap)
    tables = []
    for _ in range(2):
        out = Guarded((4 + cap * 12, 1))
        ws = GuardedWorkspace(nbytes)
        ws.fill(0xA5)
        assert lib.unetk_guide_components(acc.ptr(), guide.ptr(), h, w, cap, out.ptr(), ws.ptr(), nbytes, _stream()) == 0
        torch.cuda.synchronize()
        assert out.check_untouched() and ws.guard_intact()
        assert acc.changed_anywhere() == 0 and guide.changed_anywhere() == 0
        n = int(out.view.view(torch.int32)[0, 0])
        assert 0 < n < cap and out.unwritten() == (cap - n) * 12
        tables.append(out.view.view(torch.int32)[:4 + n * 12].clone())
    assert torch.equal(tables[0], tables[1])


def test_components_refuses_histogram_indices_past_int32():
    """cap * H and cap * W must stay below 2^31 (the histograms are indexed in int): the query returns 0, the call refuses."""
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    assert lib.unetk_guide_components_ws_bytes(40000, 10, 65536) == 0
    assert lib.unetk_guide_components_ws_bytes(10, 40000, 65536) == 0
    assert lib.unetk_guide_components_ws_bytes(40000, 10, 1024) > 0
    buf = torch.zeros(16, dtype=torch.float32, device="cuda")
    assert lib.unetk_guide_components(buf.data_ptr(), buf.data_ptr(), 40000, 10, 65536, buf.data_ptr(), buf.data_ptr(), 1 << 40,
                                      _stream()) == -1                          # UNETK_E_BADARG, nothing launched


def test_render_matches_the_formula_guard_bands_and_repeatability():
    from boxsegliver_amd import _abi
    from boxsegliver_amd.data import propagate
    rng = np.random.default_rng(5)
    for h, w, n in ((256, 256, 7), (48, 40, 1), (33, 65, 0)):
        obj = np.concatenate([rng.integers(-5, max(h, w), (n, 2)), rng.uniform(2., 9., (n, 2))], 1).astype(np.float32)
        outs = []
        for _ in range(2):
            out = Guarded((h, w, 1))
            objd = guarded_input(torch.from_numpy(obj).cuda()) if n else None
            assert _abi.lib().unetk_guide_render(objd.ptr() if n else None, n, h, w, 0.85, out.ptr(), _stream()) == 0
            torch.cuda.synchronize()
            assert out.check_untouched() and out.unwritten() == 0
            assert objd is None or objd.changed_anywhere() == 0
            outs.append(out.view[..., 0].clone())
        assert torch.equal(outs[0], outs[1])
        # float32 tolerance: expf on the device and numpy's exp may differ by a few ulp (about 6e-8 near 1)
        np.testing.assert_allclose(outs[0].cpu().numpy(), propagate.render_numpy(obj, (h, w), 0.85), rtol=0, atol=5e-7)
        if n == 0:
            assert torch.all(outs[0] == 0.5)


# ------------------------------------------------------------------------------------------------ the evaluation
def _nii_dataset(root, pids=(0, 1, 2, 3, 4, 5), depth=12, size=96, noise=True):
    """NIfTI cases with liver and two tumours each, their meta.json by extract.process_case, k_folds.txt and prior.json;
    noise=False: a constant -100 HU background instead of random values."""
    from boxsegliver_amd.data import extract, nii_kits
    rng = np.random.RandomState(5)
    (root / "nii").mkdir(parents=True, exist_ok=True)
    aff = np.array([[-0.8, 0, 0, 0], [0, -0.8, 0, 0], [0, 0, 2.5, 0], [0, 0, 0, 1.0]])
    metas = []
    for pid in pids:
        vol = rng.randint(-400, 500, size=(depth, size, size)).astype(np.int16)
        if not noise:
            vol[:] = -100
        lab = np.zeros((depth, size, size), np.uint8)
        lab[2:depth - 2, 20:70, 24:72] = 1
        lab[3:8, 30:40, 36:44] = 2
        lab[5:9, 52:60, 50:62] = 2
        vol[lab == 2] = 200
        vol[lab == 1] = 60
        v, s = root / "nii" / "volume-{}.nii".format(pid), root / "nii" / "segmentation-{}.nii".format(pid)
        nii_kits.write_nii(vol, None, v, np.int16, affine=aff)
        nii_kits.write_nii(lab, None, s, np.uint8, affine=aff)
        metas.append(extract.process_case(v, root / "png", only_meta=True))
    (root / "meta.json").write_text(json.dumps(metas))
    (root / "k_folds.txt").write_text("Fold 0:0 3\nFold 1:1 4\nFold 2:2 5\n")
    extract.write_user_prior(root)
    return metas


def _features(root, pids=(0, 1, 2, 3, 4, 5), depth=12):
    for mode in ("train", "eval"):
        d = root / "feat" / "hist" / mode
        d.mkdir(parents=True, exist_ok=True)
        for pid in pids:
            np.save(d / "{:03d}.npy".format(pid), np.full((depth, 200), 0.01 * (pid + 1), np.float32))


def _host_components(acc, guide, cap=1024, table=None, ws=None):
    """A host-driven stand-in for ops.guide_components: the table the kernel would write, from components_numpy on the
    host copies of the same probabilities and the same device guide."""
    from boxsegliver_amd.data import propagate
    a, g = acc.cpu().numpy(), guide.cpu().numpy()
    comps = propagate.components_numpy(np.argmax(a, -1) == 2, g)
    t = np.zeros(4 + cap * 12, np.int32)
    t[0], t[1] = len(comps), int(len(comps) > cap)
    for k, c in enumerate(comps[:cap]):
        row = t[4 + 12 * k:4 + 12 * k + 12]
        row[:7] = [c.root, c.area, c.box[0], c.box[1], c.box[2], c.box[3], c.peak[0] * a.shape[1] + c.peak[1]]
        row.view(np.float32)[7:] = [c.peak_value, c.center[0], c.center[1], c.stddev[0], c.stddev[1]]
    table.copy_(torch.from_numpy(t))
    return table


def _evaluator(root, run, **over):
    from boxsegliver_amd.core import models
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    argv = ("liver --mode eval --tag gsp --model GUNet --model_config GUNet_SP.yml --classes Liver Tumor --test_fold 2 "
            "--im_height 32 --im_width 32 --im_channel 3 --use_spatial --eval_mirror --random_flip 3 --evaluator Volume "
            "--normalizer instance_norm").split() + ["--lits_root", str(root), "--model_dir", str(run)]
    args, _, _ = entry.get_arguments(argv, guided=True)
    for k, v in over.items():
        setattr(args, k, v)
    params = {"args": args, "lits_root": root}
    params.update(models.get_model_params(args))
    return ev.get_evaluator("Volume", estimator=None, model_dir=str(run), params=params)


def _tumour_where_guided(loop, feats):
    """A stand-in network for the loop comparison: tumour where the centre channel is bright (the synthetic tumours) AND
    the guide is above 0.6, liver on liver intensities, background elsewhere -- per pixel, so mirrors stay consistent, and
    guided: the propagation then keeps, carries and ends tumours."""
    img, g = feats["images"][..., 1], feats["sp_guide"][..., 0]
    t = ((img > 0.8) & (g > 0.6)).float()
    liv = ((img > 0.5) & (img < 0.7)).float() * (1 - t)
    p2 = 0.8 * t + 0.1
    p1 = 0.8 * liv + 0.05
    return torch.stack([1 - p1 - p2, p1, p2], dim=-1).contiguous()


def test_device_loop_makes_the_host_loops_decisions(tmp_path, monkeypatch):
    """run_g on the device and with the components computed on the host from the same probabilities and the same device
    guides: the same objects, components and decisions on every slice, and the same volumes and metrics -- with
    probabilities that make the propagation keep and end tumours, so the decisions are not all empty."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.evaluators import evaluator_liver as evl
    _nii_dataset(tmp_path, noise=False)
    monkeypatch.setattr(evl._GuidedLoop, "_forward", _tumour_where_guided)
    ev = _evaluator(tmp_path, tmp_path / "run", im_height=64, im_width=64)
    trace_d, trace_h = [], []
    res_d = ev.run_g(checkpoint_path=None, trace=trace_d)
    monkeypatch.setattr(ops, "guide_components", _host_components)
    res_h = ev.run_g(checkpoint_path=None, trace=trace_h)
    assert len(trace_d) == len(trace_h) > 0
    for a, b in zip(trace_d, trace_h):
        assert a[:2] == b[:2] and a[4] == b[4] and a[5] == b[5]
        np.testing.assert_array_equal(a[2], b[2])
        assert [(c.root, c.area, c.box, c.peak) for c in a[3]] == [(c.root, c.area, c.box, c.peak) for c in b[3]]
        for c, d in zip(a[3], b[3]):
            np.testing.assert_array_equal(c.center, d.center)
            np.testing.assert_array_equal(c.stddev, d.stddev)
    decisions = [d for t in trace_d for d in t[4]]
    assert any(isinstance(d, int) for d in decisions) and "ended" in decisions, decisions
    assert sum(1 for t in trace_d if len(t[2]) > 0) > 2                     # objects carried over several slices
    assert res_d == res_h
    assert {"Liver/Dice", "Tumor/Dice"} <= set(res_d) and res_d["Tumor/Dice"] > 0


_TRAIN = ("liver --mode train --tag gsp --model GUNet --classes Liver Tumor --test_fold 2 "
          "--im_height 32 --im_width 32 --im_channel 3 --noise_scale 0.05 --zoom_scale 1.0 1.25 --random_flip 3 --num_of_steps 4 "
          "--loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 --batches_per_epoch 2 --batch_size 4 "
          "--weight_decay_rate 0.000001 --learning_rate 0.001 --normalizer instance_norm --use_spatial --spatial_random 1.0 "
          "--log_step 1")
_EVAL = ("liver --mode eval --tag gsp --model GUNet --classes Liver Tumor --test_fold 2 --im_height 32 --im_width 32 "
         "--im_channel 3 --normalizer instance_norm --use_spatial --eval_mirror --random_flip 3 --evaluator Volume --eval_final "
         "--metrics_eval Dice VOE")


@pytest.mark.parametrize("context,no_sp", [(False, False), (True, False), (False, True)])
def test_main_g_liver_evaluates_by_guide_propagation_end_to_end(tmp_path, context, no_sp):
    """Train a small GUNet with --use_spatial, then `main_g liver --mode eval --use_spatial --eval_mirror --random_flip 3`
    [--use_context --context_list hist 200] [--eval_no_sp]: every run finishes with per-case metrics; the propagated
    segmentation equals what the host-driven loop makes from the same checkpoint."""
    from test_gpu_lits import _write_dataset
    from boxsegliver_amd import ops
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_g
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    _write_dataset(tmp_path / "png_set")
    _nii_dataset(tmp_path / "nii_set")
    ctx = ["--use_context", "--context_list", "hist", "200"] if context else []
    cfg = ["--model_config", "GUNet_BOTH.yml" if context else "GUNet_SP.yml"]
    if context:
        from test_gpu_lits_context import _write_features
        _write_features(tmp_path / "png_set")
        _features(tmp_path / "nii_set")
    run = tmp_path / "run"
    assert main_g.main(_TRAIN.split() + cfg + ctx + ["--lits_root", str(tmp_path / "png_set"), "--model_dir", str(run)]) == 0
    argv = _EVAL.split() + cfg + ctx + ["--lits_root", str(tmp_path / "nii_set"), "--model_dir", str(run)] + \
        (["--eval_no_sp"] if no_sp else [])
    args, sub, pipe = entry.get_arguments(argv, guided=True)
    seen = {}
    orig = ev.EvaluateVolume.append_metrics

    def spy(self, results):
        seen.setdefault("cases", []).append(dict(results))
        return orig(self, results)

    ev.EvaluateVolume.append_metrics = spy
    volumes = []
    orig_score = ev.EvaluateVolume._score_case_device

    def keep(self, volume, *a, **k):
        volumes.append(np.array(volume))
        return orig_score(self, volume, *a, **k)

    ev.EvaluateVolume._score_case_device = keep
    try:
        results = entry.run(args, sub, pipe, guided=True)
        assert len(seen["cases"]) == 2 and all("Tumor/Dice" in c and "Liver/VOE" in c for c in seen["cases"])
        assert np.isfinite(results["Liver/Dice"]) and np.isfinite(results["Tumor/Dice"])
        if not no_sp:
            dev = list(volumes)
            volumes.clear()
            saved = ops.guide_components
            ops.guide_components = _host_components
            try:
                args2, sub2, pipe2 = entry.get_arguments(argv, guided=True)
                assert entry.run(args2, sub2, pipe2, guided=True) == results
            finally:
                ops.guide_components = saved
            assert len(dev) == len(volumes) == 2
            for a, b in zip(dev, volumes):
                np.testing.assert_array_equal(a, b)
    finally:
        ev.EvaluateVolume.append_metrics = orig
        ev.EvaluateVolume._score_case_device = orig_score
    assert os.path.isdir(str(run))
