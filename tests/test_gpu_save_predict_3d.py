"""GPU: --save_predict on the sliding-window 3-D evaluation (EvaluateVolume.run_3d, `liver_3d --mode eval --eval_in_patches`):
one `predict-<case>.nii.gz` per validation case, whose box is the whole case at source resolution.  The PNG store has no
NIfTI volumes, so the header is built from meta.json (nii_kits.header_from_meta); with volume files named by `vol_case`
the header is the file's.  Read back, each file equals the post-processed volume that run_3d scored."""
import json

import numpy as np
import pytest

import lits3d_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A four-step UNet3D on lits3d_ref's dataset, as in test_gpu_eval3d.py; -> (root, argv of the evaluation)."""
    from boxsegliver_amd.entry import main as entry
    root = tmp_path_factory.mktemp("save3d")
    ref.write_dataset(root)
    argv = ("liver_3d --mode train --tag cli3d --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 4 --batches_per_epoch 2 --evaluator Volume --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --log_step 1").split()
    argv += ["--lits_root", str(root), "--model_dir", str(root / "run")]
    assert entry.main(argv) == 0
    ev = list(argv)
    ev[ev.index("--mode") + 1] = "eval"
    ev[ev.index("--batch_size") + 1] = "8"
    ev += "--eval_in_patches --eval_final --save_predict".split()
    return root, ev


def _evaluate(ev, monkeypatch, save_path):
    """Run the evaluation; -> (results, {case: Liver + Tumor of the dict that reached the scoring step})."""
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.evaluators import evaluator_liver
    scored = []
    real = evaluator_liver.EvaluateVolume._score_case_device

    def recording(self, volume, labels, post_processed, accumulator, use_global):
        assert post_processed and set(volume) == {"Liver", "Tumor"}
        scored.append((volume["Liver"] + volume["Tumor"]).cpu().numpy())
        return real(self, volume, labels, post_processed, accumulator, use_global)
    monkeypatch.setattr(evaluator_liver.EvaluateVolume, "_score_case_device", recording)
    args, sub, pipe = entry.get_arguments(ev + ["--save_path", save_path])
    results = entry.run(args, sub, pipe)
    monkeypatch.undo()
    assert len(scored) == 2
    return results, dict(zip(("2", "3"), scored))


def test_3d_predictions_are_saved_with_the_fallback_header(trained, monkeypatch):
    from boxsegliver_amd.data import nii_kits
    root, ev = trained
    results, scored = _evaluate(ev, monkeypatch, "fallback")
    out = root / "run" / "fallback"
    assert sorted(p.name for p in out.iterdir()) == ["predict-2.nii.gz", "predict-3.nii.gz", "results.json"]
    assert json.loads((out / "results.json").read_text()) == results and np.isfinite(results["Liver/Dice"])
    for case, want in scored.items():
        depth = ref.DEPTHS[int(case)]
        assert want.shape == (depth, ref.H, ref.W) and want.max() <= 2
        hdr, got = nii_kits.read_nii(out / "predict-{}.nii.gz".format(case))
        np.testing.assert_array_equal(got, want)                     # unflipped: file index (x, y, z) of the data
        np.testing.assert_array_equal(nii_kits.load(out / "predict-{}.nii.gz".format(case))[1], want.transpose(2, 1, 0))
        assert hdr.shape == (ref.W, ref.H, depth) and hdr.dtype == np.int16
        np.testing.assert_allclose(hdr.pixdim, (0.8, 0.8, 2.5), rtol=1e-7)
        np.testing.assert_allclose(hdr.sform, np.diag([-0.8, -0.8, 2.5, 0.0])[:3], rtol=1e-7)


def test_3d_predictions_take_the_header_of_the_volume_file(trained, monkeypatch):
    from boxsegliver_amd.data import nii_kits
    root, ev = trained
    meta = json.loads((root / "meta.json").read_text())
    before = (root / "meta.json").read_text()
    aff = np.array([[0.7, 0, 0, -100.0], [0, -0.9, 0, 50.0], [0, 0, -3.0, 12.5]])          # x and z flipped against LiTS
    (root / "nii").mkdir()
    for case in meta:
        d, h, w = case["size"]
        case["vol_case"] = str(root / "nii" / "volume-{}.nii".format(case["PID"]))         # absolute: any proj_root
        nii_kits.write_nii(np.zeros((d, h, w), np.int16), None, case["vol_case"], np.int16, affine=aff)
    (root / "meta.json").write_text(json.dumps(meta))
    try:
        _, scored = _evaluate(ev, monkeypatch, "headers")
    finally:
        (root / "meta.json").write_text(before)
    for case, want in scored.items():
        got = root / "run" / "headers" / "predict-{}.nii.gz".format(case)
        hdr = nii_kits.load_header(got)
        vol_hdr = nii_kits.load_header(root / "nii" / "volume-{}.nii".format(case))
        assert hdr.shape == vol_hdr.shape and hdr.pixdim == vol_hdr.pixdim
        np.testing.assert_array_equal(hdr.sform, vol_hdr.sform)
        np.testing.assert_array_equal(nii_kits.read_nii(got)[1], want)
        np.testing.assert_array_equal(nii_kits.load(got)[1], np.flip(want, axis=(0, 2)).transpose(2, 1, 0))
