"""GPU: per-lesion detection on the device -- the table of unetk_component_overlaps (csrc/evalvol.hip)
against scipy.ndimage.label, np.unique and np.bincount on the CPU, integer for integer, with guard bands round the table
and the workspace; ops.component_overlaps; loss_metrics.tumor_detection_metrics_device against the host function; and
EvaluateVolume with --eval_detection under both metrics_on settings."""
import math

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import detection_ref as dref
from guardbuf import GuardedWorkspace

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x5A)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _expected(res, ref, cap_obj, cap_pair):
    """The table the kernel must leave, from scipy and numpy."""
    lres, lref, res_sizes, ref_sizes, pairs = dref.label_tables(res, ref)
    n_res, n_ref, n_pair = len(res_sizes), len(ref_sizes), len(pairs)
    over = (n_res > cap_obj) | (n_ref > cap_obj) << 1 | (n_pair > cap_pair) << 2
    table = np.zeros(4 + 4 * cap_obj + 3 * cap_pair, np.int32)
    table[:4] = [n_res, n_ref, n_pair, over]
    for k, (lab, sizes) in enumerate(((lres, res_sizes), (lref, ref_sizes))):
        ids, roots = np.unique(lab.ravel(), return_index=True)               # the first voxel of every label
        roots = roots[ids > 0]
        rows = table[4 + 2 * cap_obj * k:4 + 2 * cap_obj * (k + 1)].reshape(cap_obj, 2)
        m = min(len(sizes), cap_obj)
        rows[:m, 0], rows[:m, 1] = roots[:m], sizes[:m]
    if not over:
        table[4 + 4 * cap_obj:].reshape(cap_pair, 3)[:n_pair] = pairs
    return table


def _run(res, ref, cap_obj, cap_pair, fill=0x5A):
    """One raw call with a guarded table and a guarded workspace of exactly the queried size -> the int32 table."""
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    d, h, w = res.shape
    r, f = _dev((np.asarray(res) != 0).astype(np.uint8) * 255), _dev(np.asarray(ref).astype(np.uint8))
    words = 4 + 4 * cap_obj + 3 * cap_pair
    nbytes = lib.unetk_component_overlaps_ws_bytes(d, h, w, cap_obj, cap_pair)
    assert nbytes > 0
    table, ws = GuardedWorkspace(4 * words), GuardedWorkspace(nbytes)
    table.fill(0xA5)
    ws.fill(fill)
    assert lib.unetk_component_overlaps(r.data_ptr(), f.data_ptr(), d, h, w, cap_obj, cap_pair, table.ptr(), ws.ptr(), nbytes,
                                        _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert table.guard_intact() and ws.guard_intact()
    assert torch.equal(r, _dev((np.asarray(res) != 0).astype(np.uint8) * 255))          # inputs untouched
    return table.buf[table.off:table.off + 4 * words].cpu().numpy().view(np.int32)


def _check(res, ref, cap_obj=64, cap_pair=256, fills=(0x5A,)):
    want = _expected(res, ref, cap_obj, cap_pair)
    for fill in fills:
        got = _run(res, ref, cap_obj, cap_pair, fill)
        np.testing.assert_array_equal(got[:4], want[:4])
        np.testing.assert_array_equal(got, want)                 # rows past the counts included: they are zero
    return want


@pytest.fixture(scope="module")
def blobs():
    """Seeded pairs at 12 x 40 x 48 (six numbering tiles, 90 labelling blocks), shared by the tests below."""
    rng = np.random.default_rng(31)
    out = []
    for t in range(4):
        a = dref.blob(rng, (12, 40, 48), rng.uniform(0.05, 0.3), sigma=rng.uniform(0.8, 1.6))
        b = dref.blob(rng, (12, 40, 48), rng.uniform(0.05, 0.3), sigma=rng.uniform(0.8, 1.6))
        if t % 2 == 0:
            b = np.roll(a, (0, 1, -1), (0, 1, 2)) ^ b
        out.append((a, b))
    return out


# ------------------------------------------------------------------------------------------------ the table
def test_random_blobs_equal_scipy_and_numpy(blobs):
    for a, b in blobs:
        want = _check(a, b, cap_obj=512, cap_pair=1024, fills=FILLS)           # three workspace fills: nothing is read unwritten
        assert want[0] > 3 and want[1] > 3 and want[2] > 3
    rng = np.random.default_rng(7)
    for t in range(6):                                                         # no extent a multiple of a wavefront
        a = dref.blob(rng, (5, 7, 13), rng.uniform(0.1, 0.6), sigma=0.7)
        b = dref.blob(rng, (5, 7, 13), rng.uniform(0.1, 0.6), sigma=0.7)
        _check(a, b)


def test_single_plane_and_single_voxel_volumes():
    rng = np.random.default_rng(3)
    a, b = rng.random((1, 37, 50)) < 0.45, rng.random((1, 37, 50)) < 0.45     # D = 1
    want = _check(a, b, cap_obj=1024, cap_pair=1024)
    assert want[2] > 10
    one, zero = np.ones((1, 1, 1), bool), np.zeros((1, 1, 1), bool)
    assert _check(one, one)[:4].tolist() == [1, 1, 1, 0]
    assert _check(one, one)[4 + 4 * 64:4 + 4 * 64 + 3].tolist() == [1, 1, 1]
    assert _check(zero, zero)[:4].tolist() == [0, 0, 0, 0]
    assert _check(one, zero)[:4].tolist() == [1, 0, 0, 0]
    assert _check(zero, one)[:4].tolist() == [0, 1, 0, 0]


def test_empty_masks(blobs):
    a, b = blobs[1]
    empty = np.zeros_like(a)
    assert _check(empty, b, cap_obj=512)[:4].tolist()[0::2] == [0, 0]
    assert _check(a, empty, cap_obj=512)[:4].tolist()[1:3] == [0, 0]
    assert not _check(empty, empty).any()


def test_edge_and_corner_contacts_are_two_objects():
    for other in ((1, 2, 2), (2, 2, 2), (2, 1, 2), (2, 2, 1)):                # three edge contacts and a corner contact of (1, 1, 1)
        m = np.zeros((4, 4, 4), bool)
        m[1, 1, 1] = m[other] = True
        want = _check(m, m)
        assert want[:4].tolist() == [2, 2, 2, 0]
        assert want[4 + 4 * 64:4 + 4 * 64 + 6].tolist() == [1, 1, 1, 2, 2, 1]
    m = np.zeros((4, 4, 4), bool)
    m[1, 1, 1] = m[1, 1, 2] = True                                            # a face contact is one object
    assert _check(m, m)[:4].tolist() == [1, 1, 1, 0]


def test_full_cube_against_itself_is_one_pair_of_262144():
    m = np.ones((64, 64, 64), bool)
    want = _check(m, m, cap_obj=4, cap_pair=4)
    assert want[:4].tolist() == [1, 1, 1, 0]
    assert want[4:6].tolist() == [0, 262144] and want[4 + 16:4 + 16 + 3].tolist() == [1, 1, 262144]


def _comb(D, H, W):
    """One 6-connected object: full rows on every other line (the teeth), a spine along y at x = 0, planes joined at (0, 0)."""
    m = np.zeros((D, H, W), bool)
    m[:, ::2, :] = True
    m[:, :, 0] = True
    return m


def test_comb_across_every_block_boundary_against_its_cut_teeth():
    comb = _comb(6, 41, 67)                                                   # 16482 voxels: 65 labelling blocks, 5 tiles
    assert ndi.label(comb)[1] == 1
    teeth = comb.copy()
    teeth[:, :, 0] = False                                                    # every tooth (a slab through the planes) on its own
    teeth[:, :, 33] = False                                                   # ... and cut in two
    want = _check(teeth, comb, cap_obj=512, cap_pair=512)
    assert want[:4].tolist() == [21 * 2, 1, 21 * 2, 0]
    want = _check(comb, teeth, cap_obj=512, cap_pair=512)
    assert want[:4].tolist() == [1, 21 * 2, 21 * 2, 0]
    specks = np.random.default_rng(5).random(comb.shape) < 0.03
    _check(comb ^ specks, teeth | specks, cap_obj=2048, cap_pair=2048)


def test_one_reference_object_over_forty_single_voxel_results():
    ref = np.zeros((3, 20, 30), bool)
    ref[1, 2:18, 2:28] = True
    res = np.zeros_like(ref)
    res[1, 3:17:2, 3:27:5][:, :] = True                                       # 7 x 5 = 35 ...
    res[1, 4:14:2, 5] = True                                                  # ... + 5 isolated voxels
    assert ndi.label(res)[1] == 40
    want = _check(res, ref)
    assert want[:4].tolist() == [40, 1, 40, 0]
    pairs = want[4 + 4 * 64:].reshape(-1, 3)[:40]
    assert pairs[:, 0].tolist() == [1] * 40 and pairs[:, 1].tolist() == list(range(1, 41)) and pairs[:, 2].tolist() == [1] * 40


def test_overflow_sets_its_bit_keeps_the_true_counts_and_ops_raises():
    from boxsegliver_amd import ops
    five = np.zeros((2, 3, 11), bool)
    five[0, 0, ::2][:5] = True                                                # 5 objects
    big = np.ones_like(five)
    want = _check(five, big, cap_obj=4, cap_pair=8)
    assert want[:4].tolist() == [5, 1, 5, 1]
    want = _check(big, five, cap_obj=4, cap_pair=8)
    assert want[:4].tolist() == [1, 5, 5, 2]
    assert _check(five, five, cap_obj=4, cap_pair=8)[:4].tolist() == [5, 5, 5, 3]
    three = np.zeros_like(five)
    three[1, 2, ::4] = True                                                   # 3 objects, 3 pairs
    want = _check(three, big, cap_obj=4, cap_pair=2)
    assert want[:4].tolist() == [3, 1, 3, 4]
    assert want[4:10].tolist() == [55, 1, 59, 1, 63, 1]        # the object rows are complete
    assert _check(three, big, cap_obj=4, cap_pair=3)[:4].tolist() == [3, 1, 3, 0]        # exactly full is no overflow
    with pytest.raises(RuntimeError, match="cap_obj = 4 < 5 result"):
        ops.component_overlaps(_dev(five), _dev(big), cap_obj=4, cap_pair=8)
    with pytest.raises(RuntimeError, match="cap_obj = 4 < 5 reference"):
        ops.component_overlaps(_dev(big), _dev(five), cap_obj=4, cap_pair=8)
    with pytest.raises(RuntimeError, match="cap_pair = 2 < 3"):
        ops.component_overlaps(_dev(three), _dev(big), cap_obj=4, cap_pair=2)
    with pytest.raises(ValueError):
        ops.component_overlaps(_dev(three), _dev(big), cap_obj=0)
    with pytest.raises(ValueError):
        ops.component_overlaps(_dev(three), _dev(big[:1]))


def test_two_runs_give_bit_equal_tables(blobs):
    a, b = blobs[0]
    t1 = _run(a, b, 512, 1024, fill=0x00)
    t2 = _run(a, b, 512, 1024, fill=0xFF)
    assert t1.tobytes() == t2.tobytes()


def test_ops_component_overlaps_returns_the_numpy_tables(blobs):
    from boxsegliver_amd import ops
    for a, b in blobs[:2]:
        _, _, res_sizes, ref_sizes, pairs = dref.label_tables(a, b)
        got = ops.component_overlaps(_dev(a), _dev(b.astype(np.uint8) * 7))   # bool and any non-zero uint8
        for g, want in zip(got, (res_sizes, ref_sizes, pairs)):
            assert g.dtype == np.int64 and g.shape == want.shape
            np.testing.assert_array_equal(g, want)


# ------------------------------------------------------------------------------------------------ the metrics
def test_device_metrics_equal_host_metrics_key_for_key(blobs):
    from boxsegliver_amd.loss_metrics import tumor_detection_metrics, tumor_detection_metrics_device
    matched = 0
    for t, (a, b) in enumerate(blobs):
        for thresh in (0.5, 0.2):
            host = tumor_detection_metrics(a, b, thresh)
            dev = tumor_detection_metrics_device(_dev(a), _dev(b), thresh)
            assert list(dev) == list(host) and dev == host, (t, thresh, dev, host)
            assert all(type(dev[k]) is type(host[k]) for k in host)
            assert host == dref.detection_metrics(a, b, thresh)
            matched += host["tp"]
    assert matched > 0
    empty = np.zeros_like(blobs[0][0])
    for a, b in ((empty, blobs[0][1]), (blobs[0][0], empty), (empty, empty)):
        host, dev = tumor_detection_metrics(a, b), tumor_detection_metrics_device(a, b)   # numpy inputs are uploaded
        assert dev == host and (math.isinf(dev["precision"]) or math.isinf(dev["recall"]))


# ------------------------------------------------------------------------------------------------ the reference's records
def test_device_tables_through_the_matching_rule_give_the_reference_records():
    """tests/golden/ref_detection.npz (what the reference's own function matched; make_detection_fixtures.py): the device's
    roots, sizes and overlaps through array_kits.match_components give the same pairs in the same order, integer for
    integer; the Dice score is within 2 ulp of the float64 quotient of the recorded integers (one division of exact
    integers on either side)."""
    from boxsegliver_amd.utils import array_kits
    cap_obj, cap_pair = 64, 256
    matched = 0
    for name, res, ref, n_res, n_ref, rows in dref.reference_records():
        t = _run(res, ref, cap_obj, cap_pair)
        assert t[:2].tolist() == [n_res, n_ref] and t[3] == 0, name
        obj = t[4:4 + 4 * cap_obj].reshape(2, cap_obj, 2).astype(np.int64)
        res_rows, ref_rows = obj[0, :n_res], obj[1, :n_ref]                    # (first voxel, size) per object
        pairs = t[4 + 4 * cap_obj:].reshape(cap_pair, 3)[:t[2]].astype(np.int64)
        overlap = {(int(j), int(i)): int(o) for j, i, o in pairs}
        for thresh, want in rows.items():
            mapping = array_kits.match_components(res_rows[:, 1], ref_rows[:, 1], pairs, thresh)
            got = [(ref_rows[j - 1, 0], res_rows[i - 1, 0], overlap[(j, i)], ref_rows[j - 1, 1], res_rows[i - 1, 1])
                   for j, (i, _) in mapping.items()]
            np.testing.assert_array_equal(np.array(got, np.int64).reshape(-1, 5), want, err_msg="{} {}".format(name, thresh))
            for (_, score), (_, _, inter, a, b) in zip(mapping.values(), want.tolist()):
                q = 2.0 * inter / float(a + b)
                assert abs(score - q) <= 2 * np.spacing(q), (name, thresh, score, q)
            matched += len(want)
    assert matched > 100


# ------------------------------------------------------------------------------------------------ the evaluator
def _lits_args(tmp_path, **over):
    import test_gpu_unet as t
    from test_lits_eval_host import _write_dataset
    from boxsegliver_amd.NetworksV2.UNet import UNet
    _write_dataset(tmp_path, depth=9, size=96)
    kw = dict(batch_size=4, im_height=64, im_width=64, eval_mirror=False, random_flip=3, metrics_eval=["Dice"],
              use_global_dice=False, pred_type="pred", mode="eval", eval_num=-1, save_path=None, test_fold=2, filter_size=0,
              eval_skip_num=0, eval_in_patches=False, model="UNet")
    kw.update(over)
    yml = dict(t.YML, num_down_samples=3)
    return {"args": t.make_args(**kw), "model": UNet, "model_kwargs": yml, "model_args": (), "lits_root": tmp_path,
            "proj_root": tmp_path}


def test_evaluator_detection_keys_device_equals_host(tmp_path):
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    new = {"Tumor/DetTP", "Tumor/DetFP", "Tumor/DetPos", "Tumor/Precision", "Tumor/Recall"}
    params = _lits_args(tmp_path, eval_detection=True, detection_thresh=0.25)
    res = {}
    for on in ("host", "device"):
        e = ev.get_evaluator("Volume", estimator=None, model_dir=str(tmp_path), params=params, metrics_on=on)
        res[on] = e.run(lits.input_fn_eval, checkpoint_path=None)              # the same model instance: the same weights
        assert e.calls == 2
    assert new <= set(res["host"]) and set(res["device"]) == set(res["host"])
    for k in new:
        assert res["device"][k] == res["host"][k], (k, res["device"][k], res["host"][k])
    assert res["device"]["Tumor/DetPos"] == 2                                  # one labelled tumour per case
    assert all(type(res["device"][k]) is int for k in ("Tumor/DetTP", "Tumor/DetFP", "Tumor/DetPos"))
    params["args"].eval_detection = False                                      # without the flag: the keys of today
    plain = ev.get_evaluator("Volume", estimator=None, model_dir=str(tmp_path), params=params, metrics_on="device").run(
        lits.input_fn_eval, checkpoint_path=None)
    assert set(plain) == set(res["device"]) - new
    assert set(plain) == {"Liver/Dice", "Tumor/Dice", "GLiverDice", "GTumorDice"}
    for k in plain:
        assert plain[k] == res["device"][k], k
    params["args"].eval_detection, params["args"].classes = True, ["Liver"]
    with pytest.raises(ValueError, match="Tumor"):
        ev.get_evaluator("Volume", estimator=None, model_dir=str(tmp_path), params=params)
