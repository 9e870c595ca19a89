"""Host: `liver_3d --mode infer` -- the new entries and flags, which files are segmented and what they are
called, the orientation plan and the value rule of `unetk_nii_ingest` restated in numpy (infer3d_ref.py) against
nii_kits.read_nii, the refusals, the reader (with and without its thread), the saver's header sources and the header of a saved
probability volume."""
import argparse
import gzip
import itertools
import json
import struct

import numpy as np
import pytest

import infer3d_ref as iref

BASE = ("liver_3d --tag t --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 --im_width 32 "
        "--batch_size 8 --evaluator Volume").split()


def _args(mode="infer", extra=()):
    from boxsegliver_amd.entry import main as entry
    return entry.get_arguments(BASE + ["--mode", mode] + list(extra))[0]


def test_new_entries_are_bound_and_the_abi_stays():
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    assert _abi.ABI_VERSION == 10 and lib.unetk_abi_version() == 10
    for name in ("unetk_nii_ingest", "unetk_eval3d_prob"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert callable(ops.nii_ingest) and callable(ops.eval3d_prob)
    assert ops.STORE_WINDOW == (iref.LO, iref.HI, iref.SCALE) == (-250, 300, 64)
    from boxsegliver_amd.data import nii_kits
    assert {np.dtype(v).name for v in nii_kits._DTYPES.values()} == set(ops.NII_INGEST_CODES)
    assert all(nii_kits._CODES[np.dtype(k)] == v for k, v in ops.NII_INGEST_CODES.items())


def test_flags_parse_and_are_off_by_default():
    plain = _args()
    assert plain.infer_volumes is None and plain.infer_dir is None and plain.mode == "infer"
    a = _args(extra=["--infer_volumes", "a.nii", "b.nii.gz", "--infer_dir", "scans", "--pred_type", "prob"])
    assert a.infer_volumes == ["a.nii", "b.nii.gz"] and a.infer_dir == "scans" and a.pred_type == "prob"


@pytest.mark.parametrize("name,want", [("volume-30.nii.gz", ("30", True)), ("test-volume-3.nii", ("test-volume-3", False)),
                                       ("volume-27.nii", ("27", False)), ("volume-28.nii", ("28", True)),
                                       ("volume-47.nii.gz", ("47", True)), ("volume-48.nii", ("48", False)),
                                       ("some/dir/volume-007.nii", ("7", False)), ("scan.v2.nii.gz", ("scan.v2", False)),
                                       ("volume-3a.nii", ("volume-3a", False))])
def test_case_ids_follow_the_file_name(name, want):
    from boxsegliver_amd.data import lits3d
    assert lits3d.infer_case_id(name) == want


def test_a_file_that_is_no_nifti_name_is_refused():
    from boxsegliver_amd.data import lits3d
    with pytest.raises(ValueError, match="scan.png"):
        lits3d.infer_case_id("scan.png")


def _touch(path):
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(b"")
    return path


def test_files_are_found_and_sorted(tmp_path):
    from boxsegliver_amd.data import lits3d
    d = tmp_path / "scans"
    for name in ("b.nii", "a.nii.gz", "volume-3.nii", "notes.txt", "c.nii.bak"):
        _touch(d / name)
    one = _touch(tmp_path / "z" / "first.nii")
    files = lits3d.infer_files(_args(extra=["--infer_dir", str(d)]), {})
    assert [f.name for f in files] == ["a.nii.gz", "b.nii", "volume-3.nii"]
    files = lits3d.infer_files(_args(extra=["--infer_volumes", str(one), "--infer_dir", str(d)]), {})
    assert [f.name for f in files] == ["first.nii", "a.nii.gz", "b.nii", "volume-3.nii"]          # given order, then the directory
    with pytest.raises(FileNotFoundError, match="gone.nii"):
        lits3d.infer_files(_args(extra=["--infer_volumes", str(one), str(tmp_path / "gone.nii")]), {})
    with pytest.raises(FileNotFoundError, match="nowhere"):
        lits3d.infer_files(_args(extra=["--infer_dir", str(tmp_path / "nowhere")]), {})
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="No valid dataset"):
        lits3d.infer_files(_args(extra=["--infer_dir", str(tmp_path / "empty")]), {})
    _touch(d / "a.nii")
    with pytest.raises(ValueError, match="share a case id"):
        lits3d.infer_files(_args(extra=["--infer_dir", str(d)]), {})


def test_without_a_flag_the_folds_volume_files_are_taken(tmp_path):
    import lits3d_ref as ref
    from boxsegliver_amd.data import lits3d
    ref.write_dataset(tmp_path)
    meta = json.loads((tmp_path / "meta.json").read_text())
    for case in meta:
        case["vol_case"] = "nii/volume-{}.nii".format(case["PID"])
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    params = {"lits_root": str(tmp_path), "proj_root": str(tmp_path)}
    with pytest.raises(FileNotFoundError, match="volume-2.nii"):
        lits3d.infer_files(_args(), params)
    for pid in (2, 3):
        _touch(tmp_path / "nii" / "volume-{}.nii".format(pid))
    assert [f.name for f in lits3d.infer_files(_args(), params)] == ["volume-2.nii", "volume-3.nii"]     # test_fold 1


def test_refusals():
    from boxsegliver_amd.data import lits3d
    for mode in ("train", "eval"):
        for extra in (["--infer_volumes", "a.nii"], ["--infer_dir", "d"]):
            with pytest.raises(ValueError, match="--mode infer"):
                lits3d.check_args(_args(mode, extra + ["--eval_in_patches"]))
    with pytest.raises(NotImplementedError, match="main_eval_3d") as e:
        lits3d.check_args(_args(extra=["--use_spatial"]))
    assert "--mode infer with --use_spatial" in str(e.value)
    with pytest.raises(NotImplementedError, match="main_eval_3d") as e:
        lits3d.check_args(_args(extra=["--use_spatial", "--slice_prior", "boundary", "--im_channel", "2"]))
    assert "--slice_prior" in str(e.value)
    assert lits3d.check_args(_args()) == (2, 2)
    with pytest.raises(ValueError, match="--mode infer"):                                   # the mode and the flags disagree
        lits3d.input_fn_infer("infer", {"args": _args("eval", ["--eval_in_patches"])})
    with pytest.raises(NotImplementedError, match="mode infer with --mode eval"):           # input_fn_eval routes by both
        lits3d.input_fn_eval("infer", {"args": _args("eval", ["--eval_in_patches"])})


# ------------------------------------------------------------------------------------------------- orientation and values
def test_the_48_orientations_are_all_different():
    from boxsegliver_amd.data import nii_kits
    plans = set()
    for aff in iref.all_affines():
        hdr = nii_kits.Nifti1Header((3, 4, 5), np.int16, sform=aff)
        plans.add(nii_kits.file_orientation(hdr))
    assert len(plans) == 48 and {p[0] for p in plans} == set(itertools.permutations(range(3)))


@pytest.mark.parametrize("special", [False, True])
def test_orientation_plan_against_read_nii(tmp_path, special):
    """For every axis-aligned affine: the restated ingest of the raw file array, oriented by file_orientation's plan, is
    read_nii's array through the store's encoding."""
    from boxsegliver_amd.data import nii_kits
    raw = (np.arange(3 * 4 * 5, dtype=np.int16).reshape((3, 4, 5), order="F") * 7 - 200).astype(np.int16)
    for k, aff in enumerate(iref.all_affines()):
        path = tmp_path / "o{}.nii".format(k)
        iref.write_raw(path, raw, aff)
        hdr, data = nii_kits.read_nii(path, np.int16, special=special)
        trans_bk, flips = nii_kits.file_orientation(hdr, special)
        got = iref.ingest(raw, trans_bk, flips)
        assert got.shape == nii_kits.data_shape(hdr) == data.shape
        np.testing.assert_array_equal(got, iref.encode(data))


def test_oblique_affines_keep_their_message(tmp_path):
    from boxsegliver_amd.data import lits3d
    aff = iref.affine_for((0, 1, 2), (1, 1, 1))
    aff[0, 1] = 0.1
    iref.write_raw(tmp_path / "oblique.nii", np.zeros((3, 4, 5), np.int16), aff)
    with pytest.raises(ValueError, match="an axis-aligned affine expected") as e:
        lits3d.infer_plan(tmp_path / "oblique.nii")
    assert "oblique.nii" in str(e.value)


def test_value_rule():
    v = np.array([-0.7, -250.9, 0.7, 250.9, np.nan, 1e6, -1e6, 32767.9, -32768.9, 32766.5, np.inf, -np.inf])
    np.testing.assert_array_equal(iref.cast_int16(v), [0, -250, 0, 250, 0, 32767, -32768, 32767, -32768, 32766, 32767, -32768])
    hu = np.array([-32768, -251, -250, -249, 0, 299, 300, 301, 32767], np.int16)
    np.testing.assert_array_equal(iref.encode(hu), [0, 0, 0, 64, 16000, 35136, 35200, 35200, 35200])
    assert iref.encode(np.array([300]))[0] == 550 * 64 <= 65535
    # scaling as nii_kits.load applies it: float64 product and sum, slope 0 and NaN mean "no scaling"
    raw = np.array([0, 1000, 2048, 65535], np.uint16)
    np.testing.assert_array_equal(iref.values(raw, 1.0, -1024.0), [-1024, -24, 1024, 32767])
    np.testing.assert_array_equal(iref.values(raw, 0.5, -1024.0), [-1024, -524, 0, 31743])
    np.testing.assert_array_equal(iref.values(raw, 0.0, -1024.0), [0, 1000, 2048, 32767])
    np.testing.assert_array_equal(iref.values(raw, float("nan"), 5.0), [0, 1000, 2048, 32767])
    # in range the restatement is numpy's own cast, which is what read_nii does
    rng = np.random.default_rng(2)
    x = rng.uniform(-32768, 32767, 4096)
    np.testing.assert_array_equal(iref.cast_int16(x), x.astype(np.int16))


@pytest.mark.parametrize("dtype,slope,inter", [(np.int16, 0.0, 0.0), (np.uint8, 1.0, -1024.0), (np.uint16, 0.5, -1024.0),
                                               (np.int32, 1.0, -1024.0), (np.float32, 0.5, -1024.0), (np.float64, 0.0, 0.0)])
def test_restatement_against_read_nii_for_every_datatype(tmp_path, dtype, slope, inter):
    """Values for which numpy defines the cast: read_nii + encode is the restatement, scaling included."""
    from boxsegliver_amd.data import nii_kits
    rng = np.random.default_rng(5)
    info_hi = 255 if dtype == np.uint8 else 3000
    raw = rng.integers(0 if np.dtype(dtype).kind == "u" else -1500, info_hi, (5, 4, 3)).astype(dtype)
    if np.dtype(dtype).kind == "f":
        raw = (raw + rng.integers(-3, 4, raw.shape) / 4.0).astype(dtype)                    # fractional, negatives included
    aff = iref.affine_for((1, 2, 0), (-1, 1, -1))
    iref.write_raw(tmp_path / "v.nii.gz", raw, aff, slope, inter)
    hdr, data = nii_kits.read_nii(tmp_path / "v.nii.gz", np.int16)
    assert hdr.scl_slope == slope and hdr.scl_inter == inter
    np.testing.assert_array_equal(iref.ingest(raw, *nii_kits.file_orientation(hdr), slope=slope, inter=inter), iref.encode(data))


# ------------------------------------------------------------------------------------------------- the reader
def _volume(tmp_path, name, shape=(6, 5, 4), seed=0):
    raw = np.random.default_rng(seed).integers(-400, 400, shape).astype(np.int16)
    iref.write_raw(tmp_path / name, raw, iref.affine_for((0, 1, 2), (-1, -1, 1)))
    return raw


def _big_endian_copy(src, dst):
    raw = bytearray(src.read_bytes())
    dims = struct.unpack("<8h", raw[40:56])
    struct.pack_into(">i", raw, 0, 348)
    struct.pack_into(">8h", raw, 40, *dims)
    struct.pack_into(">h", raw, 70, struct.unpack("<h", raw[70:72])[0])
    for off, n in ((76, 8), (108, 3), (256, 3), (268, 3), (280, 12)):
        struct.pack_into(">{}f".format(n), raw, off, *struct.unpack("<{}f".format(n), raw[off:off + 4 * n]))
    struct.pack_into(">2h", raw, 252, *struct.unpack("<2h", raw[252:256]))
    dst.write_bytes(bytes(raw))


def test_plan_and_refused_files(tmp_path):
    from boxsegliver_amd.data import lits3d
    _volume(tmp_path, "volume-30.nii.gz")
    plan = lits3d.infer_plan(tmp_path / "volume-30.nii.gz")
    assert (plan["case"], plan["special"], plan["file_shape"], plan["nbytes"]) == ("30", True, (6, 5, 4), 240)
    assert plan["trans_bk"] == (2, 1, 0) and plan["shape"] == (4, 5, 6) and plan["dtype"] == np.int16
    assert plan["flips"] == (True, False, False)                    # the LiTS orientation reads unflipped; `special` mirrors x
    _volume(tmp_path, "le.nii")
    _big_endian_copy(tmp_path / "le.nii", tmp_path / "be.nii")
    with pytest.raises(ValueError, match="big-endian") as e:
        lits3d.infer_plan(tmp_path / "be.nii")
    assert "be.nii" in str(e.value)
    iref.write_raw(tmp_path / "four.nii", np.zeros((3, 4, 5, 2), np.int16), iref.affine_for((0, 1, 2), (1, 1, 1)))
    with pytest.raises(ValueError, match="3-D volume"):
        lits3d.infer_plan(tmp_path / "four.nii")


@pytest.mark.parametrize("ahead", [True, False])
def test_reader_serves_the_voxel_blocks_in_order(tmp_path, ahead):
    from boxsegliver_amd.data import lits3d
    names = ["a.nii", "b.nii.gz", "c.nii", "d.nii.gz"]
    shapes = [(6, 5, 4), (9, 7, 5), (3, 2, 2), (6, 5, 4)]                                   # the staging buffers grow and are reused
    raws = [_volume(tmp_path, n, s, seed=i) for i, (n, s) in enumerate(zip(names, shapes))]
    reader = lits3d.VolumeReader([tmp_path / n for n in names], "cpu", ahead=ahead)
    try:
        for i, raw in enumerate(raws):
            plan, block = reader.get(i)
            assert block.dtype.is_floating_point is False and block.numel() == raw.size * 2 == plan["nbytes"]
            np.testing.assert_array_equal(block.numpy().view(np.int16), raw.reshape(-1, order="F"))
            reader.sent(i)
            reader.prefetch(i + 1)
            assert len(reader.jobs) == (1 if ahead and i + 1 < len(names) else 0)           # at most one case ahead
    finally:
        reader.close()


@pytest.mark.parametrize("ahead", [True, False])
def test_reader_errors_name_the_file(tmp_path, ahead):
    from boxsegliver_amd.data import lits3d
    _volume(tmp_path, "good.nii")
    _volume(tmp_path, "cut.nii")
    (tmp_path / "cut.nii").write_bytes((tmp_path / "cut.nii").read_bytes()[:400])           # ends inside its voxel block
    _volume(tmp_path, "bad.nii.gz", shape=(40, 30, 20))
    blob = (tmp_path / "bad.nii.gz").read_bytes()
    (tmp_path / "bad.nii.gz").write_bytes(blob[:len(blob) // 2])                            # the deflate stream stops half way
    _volume(tmp_path, "crc.nii.gz")
    blob = bytearray((tmp_path / "crc.nii.gz").read_bytes())
    blob[-8] ^= 0xFF                                                                        # every byte inflates; the checksum is wrong
    (tmp_path / "crc.nii.gz").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="crc.nii.gz"):
        lits3d.read_voxel_block(tmp_path / "crc.nii.gz", lits3d.infer_plan(tmp_path / "crc.nii.gz")["header"], bytearray(240))
    _volume(tmp_path, "gone.nii")
    files = [tmp_path / n for n in ("good.nii", "cut.nii", "bad.nii.gz", "gone.nii")]
    reader = lits3d.VolumeReader(files, "cpu", ahead=ahead)
    try:
        reader.get(0)
        reader.prefetch(1)
        with pytest.raises(ValueError, match="cut.nii"):
            reader.get(1)
        reader.prefetch(2)
        with pytest.raises(ValueError, match="bad.nii.gz"):
            reader.get(2)
        if ahead:
            reader.prefetch(3)                                      # the header is read here; the block by the thread, later
            reader.jobs[3][1].result()
            reader.jobs.pop(3)
        (tmp_path / "gone.nii").unlink()
        with pytest.raises(FileNotFoundError, match="gone.nii"):
            reader.get(3)
    finally:
        reader.close()


# ------------------------------------------------------------------------------------------------- saver and prob header
class _Ev(object):
    def __init__(self, root):
        self.params = {"lits_root": str(root), "proj_root": str(root)}


def test_saver_header_comes_from_the_item_first_then_from_meta(tmp_path):
    import lits3d_ref as ref
    from boxsegliver_amd.data import nii_kits
    from boxsegliver_amd.evaluators.evaluator_liver import _CaseSaver
    ref.write_dataset(tmp_path)
    saver = _CaseSaver(_Ev(tmp_path), tmp_path)
    meta_hdr, special = saver.header("2")                                                   # as before: built from meta.json
    assert not special and meta_hdr.shape == (ref.W, ref.H, ref.DEPTHS[2])
    given = nii_kits.Nifti1Header((5, 6, 7), np.float32, (1, 2, 3), sform=iref.affine_for((2, 0, 1), (1, -1, 1)))
    saver.given["2"] = (given, True)
    saver.given["my-scan"] = (given, False)
    assert saver.header("2") == (given, True) and saver.header("my-scan") == (given, False)
    assert saver.header("3")[0].shape == (ref.W, ref.H, ref.DEPTHS[3])                      # other cases still from meta.json
    with pytest.raises(ValueError, match="not in meta.json"):
        saver.header("7")
    with pytest.raises(ValueError):
        saver.header("other-scan")                                                          # neither given nor a meta.json case


def test_prob_header_fields(tmp_path):
    from boxsegliver_amd.data import nii_kits
    src = nii_kits.Nifti1Header((5, 4, 3), np.int16, (0.7, 0.9, 3.0), sform=iref.affine_for((0, 1, 2), (1, -1, -1)),
                                scl_slope=2.0, scl_inter=-1024.0)
    hdr = nii_kits.prob_header(src)
    assert (src.scl_slope, src.scl_inter, src.dtype) == (2.0, -1024.0, np.int16)            # the input's header is not touched
    assert hdr.dtype == np.uint8 and hdr.scl_slope == 1.0 / 255 and hdr.scl_inter == 0.0 and hdr.shape == src.shape
    q = np.arange(60, dtype=np.uint8) * 4 + 15
    nii_kits.save_flat(q, (5, 4, 3), hdr, tmp_path / "p.nii.gz")
    with gzip.open(tmp_path / "p.nii.gz", "rb") as f:
        raw = f.read()
    assert struct.unpack("<h", raw[70:72])[0] == 2 and struct.unpack("<h", raw[72:74])[0] == 8
    slope, inter = struct.unpack("<2f", raw[112:120])
    assert slope == np.float32(1.0 / 255) and inter == 0.0
    back, data = nii_kits.load(tmp_path / "p.nii.gz")
    np.testing.assert_array_equal(back.sform, np.asarray(src.sform, np.float32))
    np.testing.assert_array_equal(data.reshape(-1, order="F"), q.astype(np.float64) * float(np.float32(1.0 / 255)))
    assert data.min() >= 0.0 and data.max() <= 1.0 and abs(data.reshape(-1, order="F") - q / 255.0).max() < 1e-7


def test_prob_restatement_rounds_to_even_and_masks():
    acc = np.zeros((1, 1, 6, 2), np.float32)
    acc[0, 0, :, 1] = [0.5 / 255, 1.5 / 255, 2.5 / 255, 1.0, 2.0, 0.25]
    w = np.ones((1, 1, 6), np.float32)
    w[0, 0, 5] = 0.0
    t, q = iref.prob(acc, w, 1)
    assert q.reshape(-1).tolist()[3:] == [255, 255, 0] and abs(t[0, 0, 0] - 0.5) < 1e-6
    _, q = iref.prob(acc, w, 1, (0, 1, 0, 1, 3, 5))
    assert q.reshape(-1).tolist() == [0, 0, 0, 255, 255, 0]
    exact = np.array([0.5, 1.5, 2.5]) / 256.0
    acc2 = np.zeros((1, 1, 3, 1), np.float32)
    acc2[0, 0, :, 0] = exact
    t, q = iref.prob(acc2, np.full((1, 1, 3), 255.0 / 256.0, np.float32), 0)
    assert t.reshape(-1).tolist() == [0.5, 1.5, 2.5] and q.reshape(-1).tolist() == [0, 2, 2]                 # ties to even


def test_namespace_without_the_flags_is_accepted():
    """Callers that build their arguments by hand (older scripts, the interactive evaluator) have no infer flags."""
    from boxsegliver_amd.data import lits3d
    ns = argparse.Namespace(mode="eval", classes=["Liver", "Tumor"], im_channel=1, im_depth=4, im_height=32, im_width=32)
    assert lits3d.check_args(ns) == (2, 2)
