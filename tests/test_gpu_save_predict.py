"""GPU: --save_predict end to end on the 2-D volume evaluator (EvaluateVolume.run, evaluator_liver.py:998-1026
`maybe_save_case`): the files `predict-<case>.nii.gz` written from the device (unetk_nii_compose + one copy + the
background writer) carry the header of the case's volume file, are byte-identical to the ones the literal host path
writes, and hold the prediction of the written-out loop of test_gpu_lits_eval.py (argmax, zoom, merge, largest
component), padded from the liver box to the whole case.

One UNet (random weights, shared by every run through params["model_instances"]) on
test_lits_eval_host._write_dataset(depth=9, size=96); the runs every test reads are made once per module."""
import json
import logging

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

FOLD_CASES = ("2", "5")


def _params(root, share=None, **over):
    import test_gpu_unet as t
    from boxsegliver_amd.NetworksV2.UNet import UNet
    args = t.make_args(batch_size=4, im_height=64, im_width=64, eval_mirror=False, random_flip=0,
                       metrics_eval=["Dice", "VOE"], use_global_dice=False, pred_type="pred", mode="eval", eval_num=-1,
                       save_path=None, test_fold=2, filter_size=0, eval_skip_num=0, eval_in_patches=False, model="UNet")
    for k, v in over.items():
        setattr(args, k, v)
    params = {"args": args, "model": UNet, "model_kwargs": dict(t.YML, num_down_samples=3), "model_args": (),
              "lits_root": root, "proj_root": root}
    if share is not None:
        params["model_instances"] = share["model_instances"]        # the same weights in every run
    return params


def _run(root, out, params, save=True, **kw):
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    evaluator = ev.get_evaluator("Volume", estimator=None, model_dir=str(out), params=params, **kw)
    return evaluator.run(lits.input_fn_eval, checkpoint_path=None, save=save)


def _literal(params):
    """case -> (bbox, prediction padded to the case [d, h, w] with values 0 / 1 / 2, zoomed probabilities padded): the loop
    of test_gpu_lits_eval.py on the host generator."""
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.utils import array_kits as arr_ops
    model = params["model_instances"][0]
    meta = {str(c["PID"]): c for c in json.loads((params["lits_root"] / "meta.json").read_text())}
    out, slabs, case = {}, [], None
    for feats, labels in lits.input_fn_eval(params["args"].mode, params):
        if feats is not None:
            case = str(feats["names"])
            x = torch.from_numpy(np.ascontiguousarray(feats["images"])).cuda()
            model({"images": x}, "eval", **params["model_kwargs"])
            slabs.append(model.probability.cpu().numpy())
            continue
        _, _, pads, bbox, resized = labels
        prob = np.concatenate(slabs)
        slabs = []
        if pads > 0:
            prob = prob[:-pads]
        vol = np.argmax(prob, -1).astype(np.uint8)
        ori = (vol.shape[0], bbox[4] - bbox[1] + 1, bbox[3] - bbox[0] + 1)
        if resized and ori != vol.shape:
            vol = ndi.zoom(vol, np.array(ori) / np.array(vol.shape), order=0)
            prob = ndi.zoom(prob, np.array(ori + (3,)) / np.array(prob.shape), order=1)
        liver = arr_ops.get_largest_component((vol == 1) | (vol == 2), rank=3).astype(np.uint8)
        tumor = (vol == 2).astype(np.uint8) * liver
        d, h, w = meta[case]["size"]
        pad_with = ((bbox[2], d - bbox[5] - 1), (bbox[1], h - bbox[4] - 1), (bbox[0], w - bbox[3] - 1))
        out[case] = (bbox, np.pad(liver + tumor, pad_with), np.pad(prob, pad_with + ((0, 0),)))
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from test_lits_eval_host import _write_dataset
    root = tmp_path_factory.mktemp("save_predict")
    _write_dataset(root, depth=9, size=96)
    params = _params(root)
    res_dev = _run(root, root / "dev", params, volumes_on="device")
    res_host = _run(root, root / "host", _params(root, params), volumes_on="host", metrics_on="host")
    res_plain = _run(root, root / "plain", _params(root, params), save=False, volumes_on="device")
    return dict(root=root, params=params, dev=res_dev, host=res_host, plain=res_plain, literal=_literal(params))


def test_files_carry_the_volume_header_and_the_literal_prediction(runs, tmp_path):
    from boxsegliver_amd.data import nii_kits
    root = runs["root"]
    assert sorted(p.name for p in (root / "dev" / "prediction").iterdir()) == \
        ["predict-2.nii.gz", "predict-5.nii.gz", "results.json"]
    voxels = 0
    for case in FOLD_CASES:
        got = root / "dev" / "prediction" / "predict-{}.nii.gz".format(case)
        vol_hdr = nii_kits.load_header(root / "nii" / "volume-{}.nii".format(case))
        hdr, raw = nii_kits.load(got)
        assert hdr.shape == vol_hdr.shape == (96, 96, 9) and hdr.dtype == np.int16
        assert hdr.pixdim == vol_hdr.pixdim
        np.testing.assert_array_equal(hdr.sform, vol_hdr.sform)
        # the literal host path writes the same bytes
        assert got.read_bytes() == (root / "host" / "prediction" / got.name).read_bytes()
        # ... and so does the oracle, up to its gzip settings: write_nii of the padded literal prediction, read back raw
        bbox, want, _ = runs["literal"][case]
        nii_kits.write_nii(want, vol_hdr, tmp_path / "oracle.nii")
        np.testing.assert_array_equal(raw, nii_kits.load(tmp_path / "oracle.nii")[1])
        np.testing.assert_array_equal(nii_kits.read_lits(int(case), "vol", got)[1], want)
        inside = np.zeros(want.shape, bool)
        inside[bbox[2]:bbox[5] + 1, bbox[1]:bbox[4] + 1, bbox[0]:bbox[3] + 1] = True
        assert not want[~inside].any()
        voxels += int((want > 0).sum())
        print("case {}: {} liver and {} tumor voxels saved".format(case, int((want == 1).sum()), int((want == 2).sum())))
    assert voxels > 0                                                # the comparison is not one of empty volumes


def test_saving_does_not_change_the_metrics(runs):
    assert runs["dev"] == runs["plain"] and set(runs["dev"]) >= {"Liver/Dice", "Tumor/Dice", "GLiverDice", "GTumorDice"}
    assert json.loads((runs["root"] / "dev" / "prediction" / "results.json").read_text()) == runs["dev"]
    for key, value in runs["host"].items():
        assert abs(value - runs["dev"][key]) < 1e-6 * max(1.0, abs(value)), key
    assert not (runs["root"] / "plain" / "prediction").exists()


def test_infer_writes_the_same_files_without_labels(runs, tmp_path):
    from test_lits_eval_host import _write_dataset
    _write_dataset(tmp_path, depth=9, size=96)                        # the same volumes (seeded)
    for f in (tmp_path / "nii").glob("segmentation-*"):
        f.unlink()
    params = _params(tmp_path, runs["params"], mode="infer")
    assert _run(tmp_path, tmp_path / "out", params, volumes_on="device") == {}
    assert json.loads((tmp_path / "out" / "prediction" / "results.json").read_text()) == {}
    for case in FOLD_CASES:
        name = "predict-{}.nii.gz".format(case)
        assert (tmp_path / "out" / "prediction" / name).read_bytes() == (runs["root"] / "dev" / "prediction" / name).read_bytes()
    records = []
    handler = logging.Handler(level=logging.WARNING)
    handler.emit = records.append
    logging.getLogger("boxsegliver_amd").addHandler(handler)
    try:
        assert _run(tmp_path, tmp_path / "dry", _params(tmp_path, runs["params"], mode="infer"), save=False,
                    volumes_on="device") == {}
    finally:
        logging.getLogger("boxsegliver_amd").removeHandler(handler)
    assert len([r for r in records if "nothing is written" in r.getMessage()]) == 1
    assert not (tmp_path / "dry").exists()


def test_pred_type_prob_writes_npz(runs, tmp_path):
    """Probabilities are saved, not scored (the metrics compare class masks): --mode infer, as the reference is used."""
    params = _params(runs["root"], runs["params"], pred_type="prob", mode="infer")
    assert _run(runs["root"], tmp_path, params, volumes_on="device") == {}
    for case in FOLD_CASES:
        with np.load(str(tmp_path / "prediction" / "{}.npz".format(case))) as f:
            got = f["arr_0"]
        want = runs["literal"][case][2]
        assert got.shape == (9, 96, 96, 3) and got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    assert not list((tmp_path / "prediction").glob("*.nii.gz"))


def _rewrite_with_affine(root, aff):
    """The dataset's files again with another affine: the (z, y, x) arrays the pipeline reads stay what they were."""
    from boxsegliver_amd.data import nii_kits
    for path in sorted((root / "nii").glob("*.nii")):
        dtype = np.uint8 if path.name.startswith("segmentation") else np.int16
        _, data = nii_kits.read_nii(path, out_dtype=dtype)
        nii_kits.write_nii(data, None, path, dtype, affine=aff)
        np.testing.assert_array_equal(nii_kits.read_nii(path, out_dtype=dtype)[1], data)


def test_transposing_affine_round_trips(runs, tmp_path):
    from test_lits_eval_host import _write_dataset
    from boxsegliver_amd.data import nii_kits
    _write_dataset(tmp_path, depth=9, size=96)
    aff = np.array([[0, 0.8, 0, 3.0], [0, 0, -2.5, 0], [0.8, 0, 0, -7.0], [0, 0, 0, 1.0]])      # file axes (y, x, z), flips
    _rewrite_with_affine(tmp_path, aff)
    _run(tmp_path, tmp_path / "dev", _params(tmp_path, runs["params"]), volumes_on="device")
    _run(tmp_path, tmp_path / "host", _params(tmp_path, runs["params"]), volumes_on="host", metrics_on="host")
    for case in FOLD_CASES:
        got = tmp_path / "dev" / "prediction" / "predict-{}.nii.gz".format(case)
        vol_hdr = nii_kits.load_header(tmp_path / "nii" / "volume-{}.nii".format(case))
        hdr = nii_kits.load_header(got)
        assert hdr.shape == vol_hdr.shape == (9, 96, 96)          # file axis 0 runs along z: the transposed kernel
        np.testing.assert_array_equal(hdr.sform, vol_hdr.sform)
        np.testing.assert_array_equal(nii_kits.read_nii(got)[1], runs["literal"][case][1])
        assert got.read_bytes() == (tmp_path / "host" / "prediction" / got.name).read_bytes()


def test_x_mirrored_cases_invert_their_read(runs, tmp_path):
    """LiTS cases 28..47 are x-mirrored by read_lits("vol"): the written file mirrors back, so read_lits returns the
    prediction and voxel (i, j, k) of the file is voxel (i, j, k) of the volume file (the reference, which writes without
    `special`, saves these cases mirrored against their own volume)."""
    from test_lits_eval_host import _write_dataset
    from boxsegliver_amd.data import nii_kits
    _write_dataset(tmp_path, pids=(28, 29, 30), depth=9, size=96)
    (tmp_path / "k_folds.txt").write_text("Fold 0:28\nFold 1:29\nFold 2:30\n")
    params = _params(tmp_path, runs["params"])
    _run(tmp_path, tmp_path / "dev", params, volumes_on="device")
    _run(tmp_path, tmp_path / "host", _params(tmp_path, runs["params"]), volumes_on="host", metrics_on="host")
    (bbox, want, _), = _literal(params).values()
    got = tmp_path / "dev" / "prediction" / "predict-30.nii.gz"
    np.testing.assert_array_equal(nii_kits.read_lits(30, "vol", got)[1], want)
    np.testing.assert_array_equal(nii_kits.read_nii(got)[1], np.flip(want, axis=2))
    assert (want != np.flip(want, axis=2)).any()                     # the mirror is visible in this prediction
    assert got.read_bytes() == (tmp_path / "host" / "prediction" / got.name).read_bytes()


def test_a_volume_that_is_not_its_box_is_refused(runs, tmp_path):
    """Without the resize back (im_height = im_width = 64 asked of a generator that says the case was not resized) the
    volume has the network's shape, not the box's: no file with a wrong geometry is written."""
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev

    def no_resize_back(mode, params):
        for feats, labels in lits.input_fn_eval(mode, params):
            yield feats, (labels if labels is None else labels[:4] + (False,))
    evaluator = ev.get_evaluator("Volume", estimator=None, model_dir=str(tmp_path), volumes_on="device",
                                 params=_params(runs["root"], runs["params"]))
    with pytest.raises(ValueError, match="case 2 has shape"):
        evaluator.run(no_resize_back, checkpoint_path=None, save=True)
    assert not list((tmp_path / "prediction").glob("predict-*")) and not (tmp_path / "prediction" / "results.json").exists()
