"""GPU, end to end: `liver_3d --mode infer` -- NIfTI volumes in any axis-aligned orientation are ingested on
the device (`unetk_nii_ingest`), segmented in sliding windows and saved with their own header; --pred_type prob writes one
`prob-<case>-<Class>.nii.gz` per class (`unetk_eval3d_prob`).

The dataset is lits3d_ref's with the image values rounded down to multiples of 64, so that a NIfTI file can hold the same
slices as the PNG store: HU = stored / 64 - 250.  The validation fold's volumes are written under an affine that flips x and z
against the LiTS orientation, `meta.json` names them, and the evaluation over the PNG store (--mode eval --eval_in_patches) is
the reference the infer route must reproduce byte for byte."""
import json

import numpy as np
import pytest
import torch

import infer3d_ref as iref
import lits3d_ref as ref

pytestmark = pytest.mark.gpu

AFFINE = np.array([[0.7, 0, 0, -100.0], [0, -0.9, 0, 50.0], [0, 0, -3.0, 12.5]])           # x and z flipped against LiTS


def _hu(im):
    return (im.astype(np.int64) // 64 - 250).astype(np.int16)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """-> dict(root, ev = the evaluation's argv, files = the two volume files, cases)."""
    from boxsegliver_amd.data import nii_kits
    from boxsegliver_amd.entry import main as entry
    root = tmp_path_factory.mktemp("infer3d")
    cases = [((im // 64 * 64).astype(np.uint16), lab) for im, lab in ref.make_cases()]
    ref.write_dataset(root, cases)
    (root / "nii").mkdir()
    files = {2: root / "nii" / "volume-2.nii", 3: root / "nii" / "volume-3.nii.gz"}
    meta = json.loads((root / "meta.json").read_text())
    for case in meta:
        if case["PID"] in files:
            case["vol_case"] = str(files[case["PID"]])                                      # absolute: any proj_root
            nii_kits.write_nii(_hu(cases[case["PID"]][0]), None, files[case["PID"]], np.int16, affine=AFFINE)
    (root / "meta.json").write_text(json.dumps(meta))
    argv = ("liver_3d --mode train --tag cli3d --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 4 --batches_per_epoch 2 --evaluator Volume --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --log_step 1").split()
    argv += ["--lits_root", str(root), "--model_dir", str(root / "run")]
    assert entry.main(argv) == 0
    ev = list(argv)
    ev[ev.index("--batch_size") + 1] = "8"
    ev += "--eval_final --save_predict".split()
    return dict(root=root, ev=ev, files=files, cases=cases)


def _run(t, mode, save_path, extra=()):
    """One run of the entry point; -> (results, output directory, rows of window tables served)."""
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.evaluators import evaluator_liver
    argv = list(t["ev"])
    argv[argv.index("--mode") + 1] = mode
    argv += (["--eval_in_patches"] if mode == "eval" else []) + [str(e) for e in extra] + ["--save_path", save_path]
    rows = []
    real = evaluator_liver.CaseWindows3D.add

    def counting(self, store, tab, *a, **kw):
        rows.append(len(tab))
        return real(self, store, tab, *a, **kw)
    evaluator_liver.CaseWindows3D.add = counting
    try:
        args, sub, pipe = entry.get_arguments(argv)
        results = entry.run(args, sub, pipe)
    finally:
        evaluator_liver.CaseWindows3D.add = real
    return results, t["root"] / "run" / save_path, sum(rows)


def _volumes(t):
    return ["--infer_volumes", t["files"][2], t["files"][3]]


@pytest.fixture(scope="module")
def plain(trained):
    """The evaluation over the PNG store and the infer run over the two files, both saved."""
    res_eval, out_eval, rows_eval = _run(trained, "eval", "plain_eval")
    res_infer, out_infer, rows_infer = _run(trained, "infer", "plain_infer", _volumes(trained))
    return dict(res_eval=res_eval, out_eval=out_eval, res_infer=res_infer, out_infer=out_infer, rows=(rows_eval, rows_infer))


def _same_files(a, b, names):
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name


PREDICTS = ["predict-2.nii.gz", "predict-3.nii.gz"]


def test_store_slices_equal_the_png_store(trained):
    """The premise of the byte comparisons: the ingested volume files are the stored slices, the shallow case included."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits3d
    for pid, path in trained["files"].items():
        plan = lits3d.infer_plan(path)
        assert plan["trans_bk"] == (2, 1, 0) and plan["flips"] == (True, False, True) and plan["case"] == str(pid)
        host = np.empty(plan["nbytes"], np.uint8)
        lits3d.read_voxel_block(path, plan["header"], host)
        im = ops.nii_ingest(torch.from_numpy(host).cuda(), plan["dtype"], plan["file_shape"], plan["trans_bk"], plan["flips"])
        np.testing.assert_array_equal(im.cpu().numpy().view(np.uint16), trained["cases"][pid][0])
    assert trained["cases"][2][0].shape[0] == 5                     # shallower than two windows of --im_depth 4


def test_infer_writes_the_bytes_of_the_evaluation(trained, plain):
    assert sorted(p.name for p in plain["out_infer"].iterdir()) == PREDICTS + ["results.json"]
    _same_files(plain["out_eval"], plain["out_infer"], PREDICTS)
    assert plain["rows"][0] == plain["rows"][1] > 0                 # the same windows were served
    assert plain["res_infer"] == {} and json.loads((plain["out_infer"] / "results.json").read_text()) == {}
    assert np.isfinite(plain["res_eval"]["Liver/Dice"])
    from boxsegliver_amd.data import nii_kits
    for pid, path in trained["files"].items():                      # the input file's own header and orientation
        got, src = nii_kits.load_header(plain["out_infer"] / "predict-{}.nii.gz".format(pid)), nii_kits.load_header(path)
        assert got.shape == src.shape and got.pixdim == src.pixdim and got.dtype == np.int16
        np.testing.assert_array_equal(got.sform, src.sform)
        vol = nii_kits.read_nii(plain["out_infer"] / "predict-{}.nii.gz".format(pid))[1]
        assert vol.shape == trained["cases"][pid][0].shape and set(np.unique(vol)) <= {0, 1, 2}


def test_mirrored_windows_give_the_same_bytes_too(trained, plain):
    _, out_eval, rows_eval = _run(trained, "eval", "mirror_eval", ["--eval_mirror"])
    _, out_infer, rows_infer = _run(trained, "infer", "mirror_infer", _volumes(trained) + ["--eval_mirror"])
    _same_files(out_eval, out_infer, PREDICTS)
    assert rows_eval == rows_infer == 8 * plain["rows"][0]          # --random_flip 7: the window and its seven mirrors


def test_without_a_flag_the_folds_files_are_segmented(trained, plain):
    res, out, rows = _run(trained, "infer", "fold_infer")
    _same_files(plain["out_infer"], out, PREDICTS)
    assert res == {} and rows == plain["rows"][1]


def test_another_name_and_slice_size(trained, plain, tmp_path):
    """A scan that is no LiTS case: 6 x 36 x 44, x along file axis 1 (the transposed ingest), its own spacing.  It runs behind
    a 40 x 48 case in one run, and its prediction carries its header."""
    from boxsegliver_amd.data import nii_kits
    rng = np.random.default_rng(3)
    hu = rng.integers(-300, 400, (6, 36, 44)).astype(np.int16)
    aff = iref.affine_for((1, 0, 2), (1, -1, 1), zooms=(0.6, 0.8, 2.0))
    scan = tmp_path / "scan-a.nii.gz"
    nii_kits.write_nii(hu, None, scan, np.int16, affine=aff)
    np.testing.assert_array_equal(nii_kits.read_nii(scan)[1], hu)
    res, out, rows = _run(trained, "infer", "scan_infer", ["--infer_volumes", trained["files"][3], scan, trained["files"][2]])
    assert res == {} and sorted(p.name for p in out.iterdir()) == PREDICTS + ["predict-scan-a.nii.gz", "results.json"]
    _same_files(plain["out_infer"], out, PREDICTS)                  # a case of another size in between changes nothing
    got, src = nii_kits.load_header(out / "predict-scan-a.nii.gz"), nii_kits.load_header(scan)
    assert got.shape == src.shape == (36, 44, 6) and got.pixdim == src.pixdim
    np.testing.assert_array_equal(got.sform, src.sform)
    vol = nii_kits.read_nii(out / "predict-scan-a.nii.gz")[1]
    assert vol.shape == (6, 36, 44) and set(np.unique(vol)) <= {0, 1, 2}
    # alone, the scan gives the same file: nothing of the case before it is left in the store
    _, alone, _ = _run(trained, "infer", "scan_alone", ["--infer_dir", tmp_path])
    _same_files(out, alone, ["predict-scan-a.nii.gz"])


def test_windows_restricted_to_the_box_of_the_first_run(trained, plain):
    """--eval_box_from the first infer run: nothing outside the box, inside it the bytes of the evaluation over the PNG store
    with the same box (the windows of a box are other windows than the whole case's, so the first run itself is no reference
    for the voxels inside), and fewer tables."""
    from boxsegliver_amd.data import lits3d, nii_kits
    box_flags = ["--eval_box_from", plain["out_infer"], "--eval_box_margin", "0", "2", "2"]
    _, out_eval, rows_eval = _run(trained, "eval", "boxed_eval", box_flags)
    res, out_infer, rows_infer = _run(trained, "infer", "boxed_infer", _volumes(trained) + box_flags)
    _same_files(out_eval, out_infer, PREDICTS)
    assert res == {} and rows_eval == rows_infer < plain["rows"][1]                         # fewer tables were served
    for pid in (2, 3):
        depth, h, w = trained["cases"][pid][0].shape
        box = lits3d.prediction_box(plain["out_infer"], str(pid), depth, (h, w), (0, 2, 2), special=False)
        assert box == lits3d.prediction_box(plain["out_infer"], pid, depth, (h, w), (0, 2, 2))
        print("case {}: box {} of {}".format(pid, box, (depth, h, w)))
        inside = np.zeros((depth, h, w), bool)
        inside[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
        vol = nii_kits.read_nii(out_infer / "predict-{}.nii.gz".format(pid))[1]
        assert vol[~inside].max(initial=0) == 0


def test_probabilities_are_saved_per_class(trained, plain, monkeypatch):
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import nii_kits
    from boxsegliver_amd.evaluators import evaluator_liver
    calls, volumes = [], []
    real_prob, real_finish = ops.eval3d_prob, evaluator_liver.CaseWindows3D.finish

    def recording_prob(acc, weight, cls, box=None, trans_bk=(2, 1, 0), flips=(False, False, False), out=None):
        calls.append((acc.clone(), weight.clone(), cls, box, tuple(trans_bk), tuple(flips)))
        return real_prob(acc, weight, cls, box, trans_bk, flips, out)

    def recording_finish(self, box=None, keep=False):
        out = real_finish(self, box, keep)
        volumes.append(out[0].cpu().numpy())
        assert keep and self.kept is not None                       # the accumulator is handed back, not dropped
        return out
    monkeypatch.setattr(ops, "eval3d_prob", recording_prob)
    monkeypatch.setattr(evaluator_liver.CaseWindows3D, "finish", recording_finish)
    res, out, _ = _run(trained, "infer", "prob_infer", _volumes(trained) + ["--pred_type", "prob"])
    monkeypatch.undo()
    names = ["prob-{}-{}.nii.gz".format(pid, cls) for pid in (2, 3) for cls in ("Liver", "Tumor")]
    assert res == {} and sorted(p.name for p in out.iterdir()) == sorted(names + ["results.json"])
    assert [c[2] for c in calls] == [1, 2, 1, 2] and len(volumes) == 2
    slope = float(np.float32(1.0 / 255))
    total = excluded = 0
    for k, pid in enumerate((2, 3)):
        src = nii_kits.load_header(trained["files"][pid])
        saved = []
        for j, cls in enumerate(("Liver", "Tumor")):
            acc, weight, ci, box, tb, flips = calls[2 * k + j]
            assert (tb, flips, box) == ((2, 1, 0), (True, False, True), None) and weight.dtype == torch.int32
            hdr, data = nii_kits.load(out / "prob-{}-{}.nii.gz".format(pid, cls))
            assert hdr.dtype == np.uint8 and hdr.shape == src.shape and hdr.pixdim == src.pixdim
            assert hdr.scl_slope == slope and hdr.scl_inter == 0.0
            np.testing.assert_array_equal(hdr.sform, src.sform)
            q = real_prob(acc, weight, ci, box, tb, flips).cpu().numpy()                    # the kernel called by hand
            np.testing.assert_array_equal(data.reshape(-1, order="F"), q.astype(np.float64) * slope)
            assert np.abs(data.reshape(-1, order="F") - q / 255.0).max() < 1e-7 and data.min() >= 0.0 and data.max() <= 1.0
            # and the restatement on the recorded accumulator, away from ties
            t, want = iref.prob(acc.cpu().numpy(), weight.cpu().numpy(), ci)
            sure = iref.file_order(np.abs((t - np.floor(t)) - 0.5) > 2.0 ** -14, tb, flips)
            np.testing.assert_array_equal(q[sure], iref.file_order(want, tb, flips)[sure])
            assert np.abs(q.astype(int) - iref.file_order(want, tb, flips).astype(int)).max() <= 1
            total += sure.size
            excluded += int((~sure).sum())
            saved.append(nii_kits.read_nii(out / "prob-{}-{}.nii.gz".format(pid, cls), out_dtype=np.float64)[1])
        probs = np.stack([1.0 - saved[0] - saved[1], saved[0], saved[1]], axis=-1)
        top = np.sort(probs, axis=-1)
        clear = top[..., -1] - top[..., -2] > 2.0 / 255
        print("case {}: {:.3f} of the voxels have a top-two gap above 2/255".format(pid, clear.mean()))
        assert clear.any()
        np.testing.assert_array_equal(np.argmax(probs, axis=-1)[clear], volumes[k][clear])
    print("prob: {} of {} voxels within 2^-14 of a tie".format(excluded, total))
    assert excluded <= 0.01 * total
    # --mode eval --pred_type prob: the same files, and the class volume is still scored
    res_eval, out_eval, _ = _run(trained, "eval", "prob_eval", ["--pred_type", "prob"])
    _same_files(out, out_eval, names)
    assert res_eval == plain["res_eval"]


def test_reader_errors_name_the_file(trained, tmp_path):
    blob = trained["files"][3].read_bytes()
    broken = tmp_path / "volume-9.nii.gz"
    broken.write_bytes(blob[:len(blob) // 2])
    with pytest.raises(ValueError, match="volume-9.nii.gz"):
        _run(trained, "infer", "broken", ["--infer_volumes", trained["files"][2], broken])
    with pytest.raises(FileNotFoundError, match="volume-77.nii"):
        _run(trained, "infer", "missing", ["--infer_volumes", trained["files"][2], tmp_path / "volume-77.nii"])
    with pytest.raises(ValueError, match="--mode infer"):
        _run(trained, "eval", "wrong_mode", _volumes(trained))
