"""GPU: `liver_3d --z_spacing MM` from the command line on lits3d_ref's dataset: training (with its online
evaluation) and `--mode eval --eval_in_patches`.  On a store whose cases all have the slice spacing MM every crop depth is
--im_depth, and the runs must give what the runs without the flag give: the same loss bits, the same first batch, the same
bytes of predict-<case>.nii.gz.  On a store of mixed spacings the flag trains and scores every case without an uncovered voxel."""
import json
import re

import numpy as np
import pytest
import torch

import lits3d_ref as ref

pytestmark = pytest.mark.gpu

MM = 2.5
MIXED = (2.5, 1.25, 2.5, 5.0)        # per case: the training fold (0, 1) and the validation fold (2, 3) each differ, one equals MM
TRAIN = ("liver_3d --mode train --tag cliz --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
         "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
         "--num_of_steps 2 --batches_per_epoch 2 --evaluator Volume --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
         "--learning_rate 0.001 --log_step 1").split()


def _losses(run):
    """The run's own loss lines: the per-step ones (three digits) and the final step's at full precision.  A log file also
    receives the lines of runs that follow in the same process (the logger keeps its handlers), so only the first
    --num_of_steps entries are the run's."""
    text = open(str(run / "logs" / "train_cliz")).read()
    return re.findall(r"loss = ([^,\s]+)", text)[:2] + re.findall(r"Loss for final step: ([^\s]+?)\.?\s", text)[:1]


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(equal, mixed, argv of the flagless training run on `equal`, which has been run: its checkpoint serves the evaluations)."""
    from boxsegliver_amd.entry import main as entry
    equal, mixed = tmp_path_factory.mktemp("zequal"), tmp_path_factory.mktemp("zmixed")
    ref.write_dataset(equal)
    ref.write_dataset(mixed)
    meta = json.loads((mixed / "meta.json").read_text())
    assert all(c["spacing"][0] == MM for c in meta)                 # lits3d_ref writes 2.5 mm slices
    for c, sz in zip(meta, MIXED):
        c["spacing"][0] = sz
    (mixed / "meta.json").write_text(json.dumps(meta))
    argv = TRAIN + ["--lits_root", str(equal), "--model_dir", str(equal / "run")]
    assert entry.main(argv) == 0
    return equal, mixed, argv


def _first_batch(argv):
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    args = entry.get_arguments(argv)[0]
    params = {"args": args, "lits_root": args.lits_root}
    feats, labels = next(lits3d.input_fn("train", params))
    ev = next(lits3d.input_fn("eval_online", params))
    return feats["images"], labels, feats["names"], ev[0]["images"], ev[1]


def test_equal_spacings_train_to_the_same_bits(roots):
    from boxsegliver_amd.entry import main as entry
    equal, _, argv = roots
    flagged = [a for a in argv]
    flagged[flagged.index("--model_dir") + 1] = str(equal / "run_z")
    flagged += ["--z_spacing", str(MM)]
    assert entry.main(flagged) == 0
    plain, got = _losses(equal / "run"), _losses(equal / "run_z")
    assert len(plain) >= 2 and plain == got and all(np.isfinite(float(v)) for v in got)          # the printed digits: the same floats
    for a, b in zip(_first_batch(argv), _first_batch(flagged)):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or torch.equal(a.view(torch.int32), b.view(torch.int32)))


def test_mixed_spacings_train_and_evaluate_online(roots):
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    _, mixed, argv = roots
    run = mixed / "run"
    flagged = [a for a in argv]
    flagged[flagged.index("--lits_root") + 1] = str(mixed)
    flagged[flagged.index("--model_dir") + 1] = str(run)
    flagged += ["--z_spacing", str(MM)] + ("--eval_per_epoch --eval_num_batches_per_epoch 1 --primary_metric Tumor/Dice "
                                           "--secondary_metric Liver/Dice --save_best").split()
    # the batches: crop depths 4 and 7 in training, 4 and 3 in the online evaluation, beside an unchanged table
    args = entry.get_arguments(flagged)[0]
    params = {"args": args, "lits_root": str(mixed)}
    feats, labels = next(lits3d.input_fn("train", params))
    assert feats["images"].shape == (2, 4, 32, 32, 1) and labels.shape == (2, 4, 32, 32) and bool(torch.isfinite(feats["images"]).all())
    plain = _first_batch([a for a in flagged if a not in ("--z_spacing", str(MM))])
    names = feats["names"].tolist()
    assert names == plain[2].tolist() and sorted(names) == [0, 1]
    rows = {pid: j for j, pid in enumerate(names)}
    assert torch.equal(feats["images"][rows[0]], plain[0][rows[0]]) and torch.equal(labels[rows[0]], plain[1][rows[0]])   # 2.5 mm: as it was
    assert not torch.equal(feats["images"][rows[1]], plain[0][rows[1]])                                                  # 1.25 mm: 7 slices
    assert entry.main(flagged) == 0
    status = json.load(open(str(run / "checkpoint")))
    assert status["global_step"] == 2
    losses = [float(v) for v in _losses(run)]
    assert len(losses) >= 2 and all(np.isfinite(v) for v in losses)


def _evaluate(argv, root, save_path, extra=()):
    from boxsegliver_amd.entry import main as entry
    ev = [a for a in argv]
    ev[ev.index("--mode") + 1] = "eval"
    ev[ev.index("--batch_size") + 1] = "8"
    ev[ev.index("--lits_root") + 1] = str(root)
    ev += "--eval_in_patches --eval_final --save_predict --save_path".split() + [save_path] + list(extra)
    args, sub, pipe = entry.get_arguments(ev)
    return entry.run(args, sub, pipe)


def test_equal_spacings_evaluate_to_the_same_bytes(roots):
    equal, _, argv = roots
    plain = _evaluate(argv, equal, "plain")
    flagged = _evaluate(argv, equal, "spaced", ["--z_spacing", str(MM)])
    assert plain == flagged
    for case in (2, 3):
        a = (equal / "run" / "plain" / "predict-{}.nii.gz".format(case)).read_bytes()
        assert len(a) > 0 and a == (equal / "run" / "spaced" / "predict-{}.nii.gz".format(case)).read_bytes()


def test_infer_takes_the_spacing_from_the_file(roots, monkeypatch):
    """--mode infer --z_spacing: a volume file whose slice spacing is MM is segmented to the bytes of the run without the flag; the
    same voxels under a header of 5 mm slices are tiled with 3-slice windows -- the z pixdim read through the file's orientation."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import nii_kits
    from boxsegliver_amd.entry import main as entry
    equal, _, argv = roots
    im = ref.make_cases()[3][0]
    hu = (im.astype(np.int64) // 64 - 250).astype(np.int16)
    files = {}
    for name, sz in (("same", MM), ("thick", 5.0)):
        (equal / name).mkdir()
        files[name] = equal / name / "scan.nii.gz"
        nii_kits.write_nii(hu, None, files[name], np.int16, affine=np.array([[0.7, 0, 0, -100.0], [0, -0.9, 0, 50.0], [0, 0, -sz, 12.5]]))

    def infer(path, save_path, extra=()):
        ev = [a for a in argv]
        ev[ev.index("--mode") + 1] = "infer"
        ev[ev.index("--batch_size") + 1] = "8"
        ev += ["--eval_final", "--save_predict", "--save_path", save_path, "--infer_volumes", str(path)] + list(extra)
        args, sub, pipe = entry.get_arguments(ev)
        entry.run(args, sub, pipe)
        return (equal / "run" / save_path / "predict-scan.nii.gz").read_bytes()
    seen = []
    real_acc = ops.eval3d_accumulate

    def recording_acc(*a, zcrop=None, zcrop_max=0, **kw):
        seen.append((None if zcrop is None else sorted(set(zcrop.cpu().tolist())), int(zcrop_max)))
        return real_acc(*a, zcrop=zcrop, zcrop_max=zcrop_max, **kw)
    monkeypatch.setattr(ops, "eval3d_accumulate", recording_acc)
    plain = infer(files["same"], "infer_plain")
    assert seen and all(s == (None, 0) for s in seen)
    del seen[:]
    assert infer(files["same"], "infer_same", ["--z_spacing", str(MM)]) == plain and len(plain) > 0
    assert seen and all(s == ([4], 4) for s in seen)
    del seen[:]
    thick = infer(files["thick"], "infer_thick", ["--z_spacing", str(MM)])
    assert seen and all(s == ([3], 3) for s in seen) and len(thick) > 0
    monkeypatch.undo()


def test_mixed_spacings_are_scored_without_an_uncovered_voxel(roots, monkeypatch):
    """Case 2 (5 slices, 2.5 mm) is tiled with 4-slice windows, case 3 (9 slices, 5 mm) with 3-slice ones; the evaluator raises
    when a voxel of a case stays uncovered, and the coverage it read is recorded here."""
    from boxsegliver_amd import ops
    equal, mixed, argv = roots
    seen, covers = [], []
    real_acc, real_predict = ops.eval3d_accumulate, ops.head_predict

    def recording_acc(probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=None, zcrop=None, zcrop_max=0):
        seen.append((int(case_depth), int(zcrop_max), sorted(set(zcrop.cpu().tolist())), tuple(box)))
        out = real_acc(probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=host_tab, zcrop=zcrop,
                       zcrop_max=zcrop_max)
        covers.append(cnt)
        return out
    monkeypatch.setattr(ops, "eval3d_accumulate", recording_acc)
    results = _evaluate(argv, mixed, "mixed", ["--z_spacing", str(MM)])            # the checkpoint of the run on `equal`
    monkeypatch.undo()
    for key in ("Liver/Dice", "Tumor/Dice"):
        assert np.isfinite(results[key]) and 0.0 <= results[key] <= 1.0, (key, results)
    assert {(d, m) for d, m, _, _ in seen} == {(ref.DEPTHS[2], 4), (ref.DEPTHS[3], 3)}
    assert all(z == [m] for _, m, z, _ in seen)
    assert all(int(c.min()) >= 1 for c in covers)                   # uncovered == 0: every voxel of both cases was hit
    assert sorted(p.name for p in (equal / "run" / "mixed").iterdir()) == ["predict-2.nii.gz", "predict-3.nii.gz", "results.json"]
