"""GPU: offline evaluation with the volumes kept on the device (EvaluateVolume(volumes_on="device"),
data/lits.input_fn_eval with params["volumes_on"] = "device") against the host path: the same slabs bit for bit, the same
segmentation volumes voxel for voxel, the same result dictionaries, and at most two volume uploads per case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

METRICS = ["Dice", "VOE", "RVD"]


def _params(tmp_path, **over):
    import test_gpu_unet as t
    from test_lits_eval_host import _write_dataset
    from boxsegliver_amd.NetworksV2.UNet import UNet
    _write_dataset(tmp_path, depth=9, size=96)
    kw = dict(batch_size=4, im_height=64, im_width=64, eval_mirror=False, random_flip=3, metrics_eval=METRICS,
              use_global_dice=False, pred_type="pred", mode="eval", eval_num=-1, save_path=None, test_fold=2, filter_size=0,
              eval_skip_num=0, eval_in_patches=False, model="UNet")
    kw.update(over)
    yml = dict(t.YML, num_down_samples=3)
    return {"args": t.make_args(**kw), "model": UNet, "model_kwargs": yml, "model_args": (), "lits_root": tmp_path,
            "proj_root": tmp_path}


def _run(params, volumes_on, **kw):
    """One evaluation; returns (results, the volumes _predict_case yielded as numpy arrays, whether they were device
    tensors).  The evaluators of one test share params and with it the model."""
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    evaluator = ev.get_evaluator("Volume", estimator=None, model_dir=str(params["lits_root"]), params=params,
                                 volumes_on=volumes_on, **kw)
    volumes, on_device = [], []
    inner = evaluator._predict_case

    def capture(*a, **k):
        for item in inner(*a, **k):
            on_device.append(torch.is_tensor(item[2]) and item[2].is_cuda)
            volumes.append(item[2].cpu().numpy() if torch.is_tensor(item[2]) else np.array(item[2]))
            yield item

    evaluator._predict_case = capture
    results = evaluator.run(lits.input_fn_eval, checkpoint_path=None)
    assert evaluator.calls == 2                                            # fold 2: cases 2 and 5
    return results, volumes, on_device


def _zoom_pairs(params):
    """(network extent, crop extent) per in-plane axis of the zoom back of every case."""
    from boxsegliver_amd.data import lits
    pairs = []
    for feats, labels in lits.input_fn_eval("eval", dict(params, volumes_on="device")):
        if feats is not None:
            shape = tuple(feats["images"].shape[1:3])
        else:
            bbox = labels[3]
            pairs.append((shape, (bbox[4] - bbox[1] + 1, bbox[3] - bbox[0] + 1)))
    return pairs


# ------------------------------------------------------------------------------------------------- slabs
@pytest.mark.parametrize("whole_slices,im_channel,size", [(False, 3, 64), (False, 1, 64), (True, 3, 64), (True, 1, 64),
                                                          (False, 3, 0), (True, 3, 0)])
def test_device_slabs_equal_host_slabs(tmp_path, whole_slices, im_channel, size):
    from boxsegliver_amd.data import lits
    params = _params(tmp_path, im_channel=im_channel, im_height=size, im_width=size, eval_mirror=True)
    params["whole_slices"] = whole_slices
    host = ((f, l) for f, l in lits.input_fn_eval("eval", params) if f is None or f["mirror"] == 0)   # not the mirrored copies
    n_slabs = n_cases = 0
    for (hf, hl), (df, dl) in zip(host, lits.input_fn_eval("eval", dict(params, volumes_on="device")), strict=True):
        if hf is None:
            assert df is None and len(hl) == len(dl) == 5
            assert np.array_equal(hl[0], dl[0]) and hl[0].dtype == dl[0].dtype
            assert tuple(hl[1:]) == tuple(dl[1:])
            n_cases += 1
        else:
            assert "mirror" not in df and set(df) == set(hf) - {"mirror"} and df["names"] == hf["names"]
            assert df["images"].is_cuda and df["images"].dtype == torch.float32
            assert torch.equal(df["images"], torch.from_numpy(np.ascontiguousarray(hf["images"])).cuda())
            n_slabs += 1
    assert n_cases == 2 and n_slabs >= 4


# ------------------------------------------------------------------------------------------------- evaluator
@pytest.mark.parametrize("eval_mirror,size", [(False, 64), (True, 64), (False, 112)])
def test_device_volumes_give_the_host_results(tmp_path, eval_mirror, size):
    """size 112: the zoom back 112 -> 96 is one of the pairs whose last sample scipy puts outside the input (a zero row and
    a zero column in every slice), which the device zoom has to reproduce."""
    from boxsegliver_amd import ops
    params = _params(tmp_path, eval_mirror=eval_mirror, im_height=size, im_width=size)
    pairs = _zoom_pairs(params)
    outside = [any((t < 0).any() for t in ops.zoom_tables(net, crop)) for net, crop in pairs]
    assert all(net != crop for net, crop in pairs)                         # every case is zoomed back
    assert all(outside) if size == 112 else not any(outside)
    host, host_vols, host_dev = _run(params, "host")
    dev, dev_vols, dev_dev = _run(params, "device")
    assert not any(host_dev) and all(dev_dev) and len(dev_dev) == 2
    for a, b in zip(host_vols, dev_vols, strict=True):
        assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b)
    if size == 112:
        assert all((v[:, -1] == 0).all() and (v[:, :, -1] == 0).all() for v in dev_vols)
    assert set(host) == set(dev) and "Liver/Dice" in host and "GTumorDice" in host
    for key in host:
        assert host[key] == dev[key], (key, host[key], dev[key])
    # the host metrics take the device volumes through one copy at the end
    both_host, _, _ = _run(params, "device", metrics_on="host")
    ref_host, _, _ = _run(params, "host", metrics_on="host")
    assert both_host == ref_host


def test_predict_mode_produces_the_same_volumes(tmp_path):
    params = _params(tmp_path, mode="predict")
    host, host_vols, _ = _run(params, "host")
    dev, dev_vols, dev_dev = _run(params, "device")
    assert host == dev and all(dev_dev)
    for a, b in zip(host_vols, dev_vols, strict=True):
        assert np.array_equal(a, b)


def test_device_volumes_upload_twice_per_case(tmp_path, monkeypatch):
    """The structural claim: with volumes_on="device" a case sends two volumes to the device (its raw crop, its labels);
    the host path sends every slab, then the prediction again and the labels."""
    params = _params(tmp_path, eval_mirror=True)
    _run(params, "host")                                                   # creates the model's variables
    uploads = []
    real = torch.from_numpy

    def counting(a):
        if a.ndim >= 3:                                                    # volumes and slabs; not the small tables
            uploads.append(a.shape)
        return real(a)

    monkeypatch.setattr(torch, "from_numpy", counting)
    _run(params, "host")
    n_host, n_slabs = len(uploads), sum(len(s) == 4 for s in uploads)
    del uploads[:]
    _run(params, "device")
    n_dev = len(uploads)
    assert n_dev <= 2 * 2 and all(len(s) == 3 for s in uploads), uploads
    assert n_slabs >= 2 * 2 * 4 and n_host >= n_slabs + 2 * 2               # 2 cases x 2 slabs x 4 mirror variants


# ------------------------------------------------------------------------------------------------- guide propagation
def test_guided_evaluation_zooms_back_on_the_device(tmp_path, monkeypatch):
    """run_g under the same switch: the propagated volume is zoomed back by unetk_zoom_nearest3d and scored in place; the
    volumes and the results equal the host zoom's.  Network 112 x 112 on a 51 x 49 liver box: one in-plane zoom has
    scipy's outside sample (asserted on the tables)."""
    import test_gpu_propagation as tp
    from boxsegliver_amd import ops
    from boxsegliver_amd.evaluators import evaluator_liver as evl
    tp._nii_dataset(tmp_path, noise=False)
    monkeypatch.setattr(evl._GuidedLoop, "_forward", tp._tumour_where_guided)
    ev = tp._evaluator(tmp_path, tmp_path / "run", im_height=112, im_width=112)
    seen = {"host": [], "device": []}
    inner = ev._predict_case_g

    def capture(*a, **k):
        for item in inner(*a, **k):
            vol = item[2]
            seen[ev.volumes_on].append((torch.is_tensor(vol) and vol.is_cuda,
                                        vol.cpu().numpy() if torch.is_tensor(vol) else np.array(vol)))
            yield item

    ev._predict_case_g = capture
    results = {}
    for where in ("host", "device"):
        ev.volumes_on = where
        results[where] = ev.run_g(checkpoint_path=None)
    assert [d for d, _ in seen["host"]] == [False, False] and [d for d, _ in seen["device"]] == [True, True]
    for (_, a), (_, b) in zip(seen["host"], seen["device"], strict=True):
        assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b)
        assert any((t < 0).any() for t in ops.zoom_tables((a.shape[0], 112, 112), a.shape))
        assert (b[:, -1] == 0).all() or (b[:, :, -1] == 0).all()
    assert results["host"] == results["device"] and results["host"]["Liver/Dice"] > 0


# ------------------------------------------------------------------------------------------------- fallbacks
def test_volumes_on_is_validated(tmp_path):
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    params = _params(tmp_path)
    with pytest.raises(ValueError):
        ev.EvaluateVolume(None, model_dir=str(tmp_path), params=params, volumes_on="bogus")
    with pytest.raises(ValueError):
        ev.get_evaluator("Volume", model_dir=str(tmp_path), params=params, volumes_on="bogus")
    assert ev.EvaluateVolume(None, model_dir=str(tmp_path), params=params).volumes_on == "host"


def test_probability_volumes_fall_back_to_the_host_path(tmp_path):
    """--pred_type prob (order-1 zoom of float volumes) is not moved: volumes_on="device" silently takes the host path.
    (--mode predict: probability volumes are written out, not scored.)"""
    params = _params(tmp_path, pred_type="prob", mode="predict")
    host, host_vols, _ = _run(params, "host")
    dev, dev_vols, dev_dev = _run(params, "device")
    assert not any(dev_dev) and host == dev
    for a, b in zip(host_vols, dev_vols, strict=True):
        assert a.dtype == np.float32 and a.ndim == 4 and np.array_equal(a, b)
