"""Host side of --save_predict (CPU): the argument checks of `unetk_nii_compose` (answered before any launch), the NIfTI
additions of data/nii_kits.py (header-only read, save of data already in file order, the header built from meta.json) and
the background writer (utils/volume_writer.py) fed from numpy buffers.  The oracle throughout is code the repository
already pins: nii_kits.write_nii / save / load."""
import ctypes
import gzip
import itertools
import os
import queue
import re
import threading

import numpy as np
import pytest

from boxsegliver_amd import _abi
from boxsegliver_amd.data import nii_kits
from boxsegliver_amd.utils import volume_writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -2


def affines():
    """All 48 axis-aligned orientations: world axis i along data axis perm[i], either way."""
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            aff = np.zeros((3, 4))
            for i in range(3):
                aff[i, perm[i]] = signs[i] * (0.75 + 0.5 * i)
            aff[:, 3] = (-12.5, 30.0, 4.25)
            yield aff


def header_for(aff, zyx_shape, dtype=np.int16):
    """A header whose file shape is what write_nii makes of a (z, y, x) array of zyx_shape."""
    trans_bk, _ = nii_kits.file_orientation(nii_kits.Nifti1Header((1, 1, 1), dtype, sform=aff))
    zooms = np.abs(aff[:3, :3]).max(axis=0)
    return nii_kits.Nifti1Header(tuple(zyx_shape[a] for a in trans_bk), dtype, zooms, sform=aff, qform_code=1,
                                 quatern=(0.0, 0.5, 0.5), qoffset=(1.0, 2.0, 3.0), qfac=-1.0)


def same_header(a, b):
    assert set(vars(a)) == set(vars(b))
    for key, value in vars(a).items():
        other = vars(b)[key]
        if value is None or other is None:
            assert value is None and other is None, key
        else:
            np.testing.assert_array_equal(np.asarray(value), np.asarray(other), err_msg=key)


# ------------------------------------------------------------------------------------------------- the entry point
def test_nii_compose_declared_bound_and_refuses_bad_arguments():
    hdr = open(os.path.join(ROOT, "include", "unetk.h")).read()
    lib = _abi.lib()
    assert re.search(r"\bunetk_nii_compose\s*\(", hdr)
    assert "unetk_nii_compose" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "unetk_nii_compose")
    assert lib.unetk_abi_version() == 10                        # an additive change
    buf = (ctypes.c_int16 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(liver=p, tumor=p, box=(2, 2, 2), origin=(0, 0, 0), case=(2, 3, 4), perm=(2, 1, 0), flips=0, dst=p):
        return lib.unetk_nii_compose(liver, tumor, box[0], box[1], box[2], origin[0], origin[1], origin[2], case[0], case[1],
                                     case[2], perm[0], perm[1], perm[2], flips, dst, None)
    # null pointers: the output, or both masks (one alone is allowed, but then the next check fires first below)
    assert call(dst=None) == BADARG
    assert call(liver=None, tumor=None) == BADARG
    # a box that lies outside the case, on either side of every axis; empty sizes
    for axis in range(3):
        origin = [0, 0, 0]
        origin[axis] = (2, 3, 4)[axis] - 2 + 1
        assert call(origin=tuple(origin)) == BADARG, axis
        origin[axis] = -1
        assert call(origin=tuple(origin)) == BADARG, axis
        box = [2, 2, 2]
        box[axis] = 0
        assert call(box=tuple(box)) == BADARG, axis
        case = [2, 3, 4]
        case[axis] = 0
        assert call(case=tuple(case)) == BADARG, axis
    assert call(box=(3, 2, 2)) == BADARG
    assert call(box=(2, 2, 2), origin=(2 ** 31 - 2, 0, 0)) == BADARG       # z1 + bd overflows 32 bits
    # trans_bk that is not a permutation of 0..2
    for perm in ((0, 0, 1), (2, 2, 2), (0, 1, 3), (-1, 1, 2), (2, 1, 1)):
        assert call(perm=perm) == BADARG, perm
    assert call(flips=8) == BADARG
    # d * h * w >= 2^31 (eio_fits): a valid request this build has no kernel for
    assert call(case=(2048, 1024, 1024)) == UNSUPPORTED
    assert call(case=(1 << 11, 1 << 10, 1 << 10), perm=(0, 1, 2)) == UNSUPPORTED
    assert call(case=(1 << 11, 1 << 10, 1 << 10), perm=(0, 1, 1)) == BADARG          # bad arguments come first
    assert all(v == 0 for v in buf)                                                   # nothing was written


# ------------------------------------------------------------------------------------------------- nii_kits
def test_header_only_read_agrees_with_load(tmp_path):
    rng = np.random.RandomState(1)
    for k, aff in enumerate(list(affines())[::5]):
        data = rng.randint(-5, 5, size=(3, 4, 5)).astype(np.int16)
        for name in ("a.nii", "a.nii.gz"):
            path = tmp_path / "{}{}".format(k, name)
            nii_kits.write_nii(data, header_for(aff, data.shape), path)
            full, _ = nii_kits.load(path)
            same_header(nii_kits.load_header(path), full)
    path = tmp_path / "u8.nii.gz"                                 # no sform: the qform / pixdim branches of the header
    nii_kits.save(np.zeros((2, 3, 4), np.uint8), nii_kits.Nifti1Header((2, 3, 4), np.uint8, (0.5, 0.6, 0.7), qform_code=1,
                                                                       quatern=(0.0, 1.0, 0.0), qfac=-1.0), path)
    same_header(nii_kits.load_header(path), nii_kits.load(path)[0])
    (tmp_path / "bad.nii").write_bytes(b"\0" * 400)
    with pytest.raises(ValueError, match="not a NIfTI-1"):
        nii_kits.load_header(tmp_path / "bad.nii")
    # a .gz is not inflated past the header: a stream cut after its first block still yields the header
    big = tmp_path / "big.nii.gz"
    nii_kits.save_flat(rng.randint(0, 3, size=200000).astype(np.int16), (200, 100, 10),
                       header_for(next(affines()), (10, 100, 200)), big)
    cut = tmp_path / "cut.nii.gz"
    cut.write_bytes(big.read_bytes()[:20000])
    assert nii_kits.load_header(cut).shape == (200, 100, 10)
    with pytest.raises(EOFError):
        nii_kits.load(cut)


def test_file_order_helpers_restate_write_nii(tmp_path):
    """to_file_order + save_flat write what write_nii writes, byte for byte, in all 48 orientations x special."""
    rng = np.random.RandomState(2)
    n = 0
    for aff in affines():
        for special in (False, True):
            data = rng.randint(0, 3, size=(5, 6, 7)).astype(np.uint8)
            hdr = header_for(aff, data.shape)
            assert nii_kits.data_shape(hdr) == (5, 6, 7)
            nii_kits.write_nii(data, hdr, tmp_path / "ref.nii", special=special)
            nii_kits.save_flat(nii_kits.to_file_order(data, hdr, special), hdr.shape, hdr, tmp_path / "got.nii")
            assert (tmp_path / "got.nii").read_bytes() == (tmp_path / "ref.nii").read_bytes()
            back = nii_kits.read_nii(tmp_path / "got.nii", special=special)[1]
            np.testing.assert_array_equal(back, data)
            n += 1
    assert n == 96
    with pytest.raises(ValueError, match="dense 1-D"):
        nii_kits.save_flat(np.zeros((2, 3), np.int16), (2, 3), hdr, tmp_path / "x.nii")
    with pytest.raises(ValueError, match="dense 1-D"):
        nii_kits.save_flat(np.zeros(5, np.int16), (2, 3), hdr, tmp_path / "x.nii")


def test_fallback_header_reads_back_unflipped(tmp_path):
    rng = np.random.RandomState(3)
    data = rng.randint(0, 3, size=(4, 5, 6)).astype(np.uint8)
    hdr = nii_kits.header_from_meta([4, 5, 6], [2.5, 0.7, 0.8])
    assert hdr.shape == (6, 5, 4) and nii_kits.data_shape(hdr) == (4, 5, 6)
    assert nii_kits.file_orientation(hdr) == ((2, 1, 0), (False, False, False))
    path = tmp_path / "p.nii.gz"
    nii_kits.save_flat(nii_kits.to_file_order(data, hdr), hdr.shape, hdr, path)
    got_hdr, back = nii_kits.read_nii(path, out_dtype=np.uint8)
    np.testing.assert_array_equal(back, data)                     # unflipped: the array index of the file is (x, y, z)
    np.testing.assert_array_equal(nii_kits.load(path)[1], data.transpose(2, 1, 0))
    np.testing.assert_allclose(got_hdr.pixdim, (0.8, 0.7, 2.5), rtol=1e-7)
    np.testing.assert_allclose(got_hdr.sform, np.diag([-0.8, -0.7, 2.5, 0])[:3], rtol=1e-7)
    np.testing.assert_array_equal(got_hdr.sform[:, 3], 0.0)


# ------------------------------------------------------------------------------------------------- the writer
def _volumes(rng, n):
    out = []
    for k in range(n):
        zyx = (3 + k, 5, 6 + k)
        aff = list(affines())[7 * k % 48]
        data = rng.randint(0, 3, size=zyx).astype(np.int16)
        out.append((data, header_for(aff, zyx)))
    return out


def test_writer_files_equal_nii_kits_save_and_are_reproducible(tmp_path):
    rng = np.random.RandomState(4)
    vols = _volumes(rng, 5)
    runs = []
    for run in ("a", "b"):
        d = tmp_path / run
        d.mkdir()
        w = volume_writer.VolumeWriter()
        paths = [d / "predict-{}.nii.gz".format(k) for k in range(len(vols))]
        for path, (data, hdr) in zip(paths, vols):
            w.submit(path, hdr, hdr.shape, nii_kits.to_file_order(data, hdr))
        w.close()
        assert w.written == [str(p) for p in paths]               # one thread: the order of submission
        assert w.max_pending <= volume_writer.MAX_PENDING and w.pending == 0
        runs.append([p.read_bytes() for p in paths])
        for path, (data, hdr) in zip(paths, vols):
            ref = tmp_path / "ref.nii.gz"
            trans_bk, _ = nii_kits.file_orientation(hdr)
            nii_kits.write_nii(data, hdr, ref)
            ref_hdr, ref_data = nii_kits.load(ref)
            got_hdr, got_data = nii_kits.load(path)
            same_header(got_hdr, ref_hdr)
            np.testing.assert_array_equal(got_data, ref_data)
            raw = path.read_bytes()
            assert raw[3] == 0 and raw[4:8] == b"\0\0\0\0"        # gzip header: no file name, mtime 0
            assert len(gzip.decompress(raw)) == 352 + 2 * data.size
    assert runs[0] == runs[1]                                     # two runs: identical bytes
    with pytest.raises(RuntimeError, match="closed"):
        w.submit(tmp_path / "late.nii.gz", vols[0][1], vols[0][1].shape, nii_kits.to_file_order(*vols[0]))


def test_writer_holds_at_most_two_cases(tmp_path, monkeypatch):
    rng = np.random.RandomState(5)
    (data, hdr), = _volumes(rng, 1)
    flat = nii_kits.to_file_order(data, hdr)
    gate, seen = threading.Event(), []
    real = nii_kits.save_flat

    def slow_save(*args, **kwargs):
        gate.wait(60)
        seen.append(w.pending)
        return real(*args, **kwargs)
    monkeypatch.setattr(nii_kits, "save_flat", slow_save)
    w = volume_writer.VolumeWriter()
    w.submit(tmp_path / "0.nii.gz", hdr, hdr.shape, flat)         # being written (held at the gate)
    w.submit(tmp_path / "1.nii.gz", hdr, hdr.shape, flat)         # queued
    with pytest.raises(queue.Full):
        w.submit(tmp_path / "2.nii.gz", hdr, hdr.shape, flat, block=False)
    assert w.pending == 2 and not (tmp_path / "0.nii.gz").exists()
    # a blocking submit waits for a place: it returns only after the gate opened
    order = []
    t = threading.Thread(target=lambda: (w.submit(tmp_path / "3.nii.gz", hdr, hdr.shape, flat), order.append("submitted")))
    t.start()
    assert order == []
    order.append("opened")
    gate.set()
    t.join(60)
    assert order == ["opened", "submitted"]
    for k in range(4, 8):
        w.submit(tmp_path / "{}.nii.gz".format(k), hdr, hdr.shape, flat)
    w.close()
    assert max(seen) <= 2 and w.max_pending == 2 and len(w.written) == 7
    assert not (tmp_path / "2.nii.gz").exists()


def test_writer_errors_reach_the_caller(tmp_path):
    rng = np.random.RandomState(6)
    (data, hdr), = _volumes(rng, 1)
    flat = nii_kits.to_file_order(data, hdr)
    missing = tmp_path / "no_such_dir"
    w = volume_writer.VolumeWriter()
    w.submit(missing / "0.nii.gz", hdr, hdr.shape, flat)
    with pytest.raises(OSError):                                   # an unwritable directory raises at close()
        w.close()
    assert w.written == []
    # ... or at the next submit, whichever comes first; the thread survives and serves what follows the report
    w = volume_writer.VolumeWriter()
    w.submit(missing / "0.nii.gz", hdr, hdr.shape, flat)
    w._queue.join()                                                 # the thread has met the error
    with pytest.raises(OSError):
        w.submit(tmp_path / "1.nii.gz", hdr, hdr.shape, flat)
    w.submit(tmp_path / "2.nii.gz", hdr, hdr.shape, flat)
    w.close()
    assert w.written == [str(tmp_path / "2.nii.gz")]
    # an exception of any kind, raised by a job of the other sort
    w = volume_writer.VolumeWriter()

    def boom():
        raise KeyError("boom")
    w.submit_call(tmp_path / "x", boom)
    with pytest.raises(KeyError, match="boom"):
        w.close()
    w.close()                                                       # reported once


# ------------------------------------------------------------------------------------------------- the evaluator's host path
class _Model(object):
    classes = ["Background", "Liver", "Tumor"]


def _host_evaluator(root, tmp_path, **cfg):
    import argparse
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    args = argparse.Namespace(**dict(dict(mode="eval", pred_type="pred", save_path=None), **cfg))
    params = {"args": args, "model_instances": [_Model()], "lits_root": root, "proj_root": root}
    return ev.EvaluateVolume(None, model_dir=str(tmp_path / "run"), params=params, metrics_on="host", volumes_on="host")


def _class_volume(rng, box):
    """Class ids with one large liver blob (tumor inside), a small detached liver speck and a detached tumor speck."""
    vol = np.zeros(box, np.uint8)
    vol[1:-1, 2:-3, 3:-2] = 1
    vol[2, 4:7, 5:9] = 2
    vol[0, 0, 0] = 1
    vol[-1, -1, -1] = 2
    return vol


@pytest.mark.parametrize("pid", [3, 30])
def test_evaluator_host_path_writes_the_padded_post_processed_mask(tmp_path, pid):
    """EvaluateVolume._run_actual with --save_predict on host volumes: header by PID from meta.json's vol_case, the mask
    post-processed once (the yielded dict is scored as it is), padded to the case and written so that read_lits returns it
    -- for the x-mirrored PIDs too."""
    import json
    from boxsegliver_amd.utils import array_kits as arr_ops
    rng = np.random.RandomState(7)
    d, h, w = 6, 20, 24
    aff = np.array([[-0.8, 0, 0, 1.0], [0, -0.8, 0, 2.0], [0, 0, 2.5, 3.0]])
    (tmp_path / "nii").mkdir()
    nii_kits.write_nii(rng.randint(-100, 100, size=(d, h, w)).astype(np.int16), None, tmp_path / "nii" / "volume-{}.nii".format(pid),
                       np.int16, affine=aff)
    meta = [{"PID": pid, "vol_case": "nii/volume-{}.nii".format(pid), "size": [d, h, w], "spacing": [2.5, 0.8, 0.8]},
            {"PID": 99, "size": "[4, 9, 11]", "spacing": "[2.0, 0.5, 0.6]"}]
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    bbox = [5, 3, 1, 20, 16, 5]                                   # x1, y1, z1, x2, y2, z2 (inclusive)
    box = arr_ops.bbox_to_shape(bbox)
    vol = _class_volume(rng, box)
    labels = (vol > 0).astype(np.uint8)
    evaluator = _host_evaluator(tmp_path, tmp_path)
    seen = []

    def predict_fn(predicts, cases=-1, dtype="pred", save_path=None):
        for case, volume, bb in predicts:
            out = evaluator._maybe_save_case(case, volume, bb, dtype, save_path)
            seen.append(out)
            yield (case, labels) + out
    results = evaluator._run_actual(predict_fn, lambda: iter([(str(pid), vol.copy(), bbox)]), True)
    (post, flag), = seen
    assert flag is True and set(post) == {"Liver", "Tumor"}
    want = np.zeros((d, h, w), np.uint8)
    liver = arr_ops.get_largest_component(vol > 0, rank=3).astype(np.uint8)
    want[1:6, 3:17, 5:21] = liver + (vol == 2) * liver
    assert want.max() == 2 and want[1, 3, 5] == 0 and (want == 2).sum() == 12           # the specks are gone
    out = tmp_path / "run" / "prediction"
    got = out / "predict-{}.nii.gz".format(pid)
    np.testing.assert_array_equal(nii_kits.read_lits(pid, "vol", got)[1], want)
    same = nii_kits.read_nii(got)[1]
    np.testing.assert_array_equal(same, np.flip(want, axis=2) if pid == 30 else want)
    same_header(nii_kits.load_header(got), nii_kits.load_header(tmp_path / "nii" / "volume-{}.nii".format(pid)))
    assert json.loads((out / "results.json").read_text()) == results and results["GLiverDice"] > 0.9
    # a case without a volume file: the header comes from meta.json (nested lists may be stored as strings)
    evaluator.config.mode = "infer"                               # no labels, no metrics: results.json stays {}
    assert evaluator._run_actual(predict_fn, lambda: iter([("99", np.ones((4, 9, 11), np.uint8), [0, 0, 0, 10, 8, 3])]), True) == {}
    assert json.loads((out / "results.json").read_text()) == {}
    hdr, back = nii_kits.read_nii(out / "predict-99.nii.gz")
    assert hdr.shape == (11, 9, 4) and np.allclose(hdr.pixdim, (0.6, 0.5, 2.0)) and back.shape == (4, 9, 11)
    # a volume that does not have its box's shape, a box that leaves the case, an unknown case: no file
    (out / "results.json").unlink()
    for case, volume, bb, match in (("99", np.ones((4, 8, 11), np.uint8), [0, 0, 0, 10, 8, 3], "case 99 has shape"),
                                    ("99", np.ones((4, 9, 11), np.uint8), [1, 0, 0, 11, 8, 3], "leaves its volume"),
                                    ("7", np.ones((4, 9, 11), np.uint8), [0, 0, 0, 10, 8, 3], "not in meta.json")):
        with pytest.raises(ValueError, match=match):
            evaluator._run_actual(predict_fn, lambda: iter([(case, volume, bb)]), True)
        assert not (out / "results.json").exists() and evaluator._saver is None


def test_evaluator_closes_the_writer_before_results_and_on_errors(tmp_path, monkeypatch):
    import json
    (tmp_path / "meta.json").write_text(json.dumps([{"PID": 1, "size": [2, 3, 4], "spacing": [1.0, 1.0, 1.0]}]))
    evaluator = _host_evaluator(tmp_path, tmp_path, save_path="out")
    labels = np.ones((2, 3, 4), np.uint8)

    def predict_fn(predicts, cases=-1, dtype="pred", save_path=None):
        for case in predicts:
            yield (case, labels) + evaluator._maybe_save_case(case, np.ones((2, 3, 4), np.uint8), [0, 0, 0, 3, 2, 1], dtype, save_path)

    def failing_save(*a, **k):
        raise OSError("disk full")
    monkeypatch.setattr(nii_kits, "save_flat", failing_save)
    with pytest.raises(OSError, match="disk full"):                # met in the thread, raised in the caller, nothing claimed
        evaluator._run_actual(predict_fn, lambda: iter(["1"]), True)
    assert (tmp_path / "run" / "out").is_dir() and not (tmp_path / "run" / "out" / "results.json").exists()
    monkeypatch.undo()
    evaluator._run_actual(predict_fn, lambda: iter(["1"]), True)
    assert sorted(p.name for p in (tmp_path / "run" / "out").iterdir()) == ["predict-1.nii.gz", "results.json"]
