"""CPU: `liver_3d --use_spatial` -- the flags, the refusals, the restatement of the 3-D click simulator
(lits3d_clicks_ref.py) against a voxel-by-voxel erosion and against what the REFERENCE itself gave on the records of
tests/click3d_shapes.py (tests/golden/ref_clicks3d.json), the records' reasons for being there, the new entry points' argument
checks, and the sampler stream of an unguided run."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import click3d_shapes as c3
import click_shapes as cs
import lits3d_clicks_ref as cref
import lits3d_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
# threed_script/201_unet_v1.sh's flag list with the sub-command and the classes changed, plus the guide flags
SCRIPT_3D = ("liver_3d --mode train --tag 201_unet_v1 --model UNet3D --classes Liver Tumor --test_fold 2 --im_depth 10 --im_height 256 "
             "--im_width 256 --im_channel 1 --random_flip 7 --num_of_total_steps 400000 --primary_metric Tumor/Dice "
             "--loss_weight_type numerical --loss_numeric_w 1 1 3 --batches_per_epoch 2000 --batch_size 4 --weight_decay_rate 0.00003 "
             "--learning_policy plateau --learning_rate 0.0003 --lr_end 0.0000005 --lr_decay_rate 0.2 --lr_patience 30 "
             "--eval_num_batches_per_epoch 200 --eval_per_epoch --evaluator Volume --normalizer instance_norm --tumor_percent 0.75 "
             "--save_best --summary_prefix liver --log_step 125 --lits_root /data/LiTS "
             "--use_spatial --local_enhance --guide_channel 2").split()


def _args(extra=""):
    from boxsegliver_amd.entry import main as entry
    return entry.get_arguments(SCRIPT_3D + extra.split())[0]


# ------------------------------------------------------------------------------------------------- flags and refusals
def test_liver_3d_parses_the_guide_flags_with_the_reference_defaults():
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    args, sub, _ = entry.get_arguments(SCRIPT_3D)
    assert sub == "liver_3d" and args.use_spatial and args.local_enhance
    assert args.stddev == [1, 3, 3] and args.guide_channel == 2
    assert lits3d.check_args(args) == (2, 2)
    assert lits3d.guide_config(args) == dict(channels=2, stddev=(1.0, 3.0, 3.0))
    plain = entry.get_arguments([a for a in SCRIPT_3D if a not in ("--use_spatial", "--local_enhance")])[0]
    assert not plain.use_spatial and not plain.local_enhance and lits3d.guide_config(plain) is None
    euclid = _args("--guide_channel 1 --stddev 2 4.5 4.5")
    euclid.local_enhance = False
    assert lits3d.guide_config(euclid) == dict(channels=1, stddev=None)
    assert lits3d.guide_stddev(_args("--stddev 2 4.5 4.5")) == (2.0, 4.5, 4.5)
    # no other flag of nf_3d came along
    for flag in ("--eval_no_sp", "--save_sp_guide", "--fp_sample", "--use_cascade", "--use_2d"):
        with pytest.raises(SystemExit):
            entry.get_arguments(SCRIPT_3D + [flag])


@pytest.mark.parametrize("extra,exc,match", [
    ("--stddev 3", ValueError, "--stddev"), ("--stddev 1 3", ValueError, "--stddev"), ("--stddev 1 3 3 3", ValueError, "--stddev"),
    ("--stddev 1 0 3", ValueError, "--stddev"), ("--stddev 1 3 -3", ValueError, "--stddev"), ("--stddev 1 nan 3", ValueError, "--stddev"),
    ("--guide_channel 0", ValueError, "--guide_channel"), ("--guide_channel 3", ValueError, "--guide_channel"),
])
def test_check_args_refuses_and_names_the_flag(extra, exc, match):
    from boxsegliver_amd.data import lits3d
    with pytest.raises(exc, match=match):
        lits3d.check_args(_args(extra))


def test_offline_evaluation_with_clicks_is_refused_and_names_the_mode():
    from boxsegliver_amd.data import lits3d
    args = _args("--eval_in_patches")
    args.mode = "eval"
    with pytest.raises(NotImplementedError, match="--mode eval with --use_spatial"):
        lits3d.check_args(args)
    with pytest.raises(NotImplementedError, match="--mode eval with --use_spatial"):
        next(lits3d.input_fn_eval("eval", {"args": args}))
    args.use_spatial = False
    assert lits3d.check_args(args) == (2, 2)


# ------------------------------------------------------------------------------------------------- the restatement
def _random_masks():
    rng = np.random.default_rng(5)
    out = []
    for t in range(8):
        d, h, w = int(rng.integers(1, 4)), int(rng.integers(6, 15)), int(rng.integers(6, 15))
        m = (rng.random((d, h, w)) < (0.5, 0.9, 0.97, 0.03)[t % 4]).astype(np.uint8)
        if t % 4 == 1:
            m[0] = 0                                                                 # a slice without an object
        out.append(m)
    return out


@pytest.mark.parametrize("margin,band", [(1, 2), (2, 3)])
def test_candidates_equal_a_voxel_by_voxel_erosion_and_the_chessboard_thresholds(margin, band):
    seen = set()
    for obj in _random_masks():
        fg = cref.candidates(obj, margin, band, False)
        np.testing.assert_array_equal(fg, cref.erode_brute(obj, margin, 0))
        g1 = cref.erode_brute(1 - obj, margin, 1)
        bg = cref.candidates(1 - obj, margin, band, True)
        np.testing.assert_array_equal(bg, g1 ^ cref.erode_brute(g1, band, 1))
        # the statement of include/unetk.h: thresholds of the chessboard distance inside each slice, nothing crosses slices
        np.testing.assert_array_equal(fg, cref.chessboard_sets(obj, margin, band, False))
        np.testing.assert_array_equal(bg, cref.chessboard_sets(1 - obj, margin, band, True))
        for z in range(obj.shape[0]):
            if not obj[z].any():
                assert not bg[z].any()                                               # no object, no background candidate
                seen.add("empty_slice")
        seen.add("fg" if fg.any() else "no_fg")
        seen.add("bg" if bg.any() else "no_bg")
    assert seen >= {"fg", "no_fg", "bg", "empty_slice"}


def test_round_half_to_even_in_integers_equals_numpy():
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(1, 40))
        v = rng.integers(0, 50, n)
        assert cref.round_half_even_mean(v.sum(), n) == int(np.round(v.mean()))
    assert [cref.round_half_even_mean(s, 2) for s in (1, 3, 5, 7)] == [0, 2, 2, 4]


# ------------------------------------------------------------------------------------------------- the records
@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "ref_clicks3d.json")) as f:
        return json.load(f)


def restated(rec):
    """(obj patch, box, pts, cnt, trace) of one record through the restatement."""
    vol = c3.build(rec["volume"])
    shape = (rec["depth"],) + tuple(rec["crop"])
    obj, box = cref.object_patch(vol, rec["centre"], rec["crop"], shape, 1)
    trace = {}
    pts, cnt = cref.clicks(obj, np.array(rec["row"], dtype=np.uint64), tuple(rec["params"]), trace)
    return obj, box, pts, cnt, trace


def test_volumes_rebuild_bit_identically(fixture):
    assert set(fixture["volumes"]) == set(c3.VOLUMES)
    for name, want in fixture["volumes"].items():
        vol = c3.build(name)
        assert list(vol.shape) == want["shape"] and c3.checksum(vol) == (want["popcount"], want["index_sum"])
    assert [(r["id"], r["row"]) for r in fixture["records"]] == [(rid, list(row)) for rid, *_, rows in c3.RECORDS for row in rows]


def test_restatement_equals_the_reference_records(fixture):
    deviations = []
    for rec in fixture["records"]:
        obj, box, pts, cnt, trace = restated(rec)
        z1, y1, x1, ch, cw = box
        assert [z1, y1, x1, z1 + rec["depth"], y1 + ch, x1 + cw] == rec["box"], rec["id"]       # the crop clamp, pinned too
        assert (rec["box_via"] == "padded") == (c3.build(rec["volume"]).shape[0] < rec["depth"])
        fg, bg = pts[0, :cnt[0]].tolist(), pts[1, :cnt[1]].tolist()
        assert fg == rec["fg"] and bg == rec["bg"], (rec["id"], rec["row"][2])
        asked = {k: [list(p) for p in zip(trace[k].get("ranks", []), trace[k].get("counts", []))] for k in ("fg", "bg")}
        assert asked == rec["asked"], (rec["id"], rec["row"][2])
        if rec["raises"]:
            deviations.append(rec["id"])
            assert obj.all() and cnt[1] == 0                                         # the deviation: no background click
    assert set(deviations) == {"all"}                                                # only the all-object patch differs


def test_records_cover_what_they_are_there_for(fixture):
    recs = {}
    for rec in fixture["records"]:
        recs[(rec["id"], rec["row"][2])] = (rec,) + restated(rec)
    assert {s for _, s in recs} == {1, 3}
    for (rid, _), (rec, obj, box, pts, cnt, trace) in recs.items():
        assert rec["row"][:2] == [4, 4]                                              # four clicks of each kind asked
        assert 0 in rec["row"][4:] and cs.LAST in rec["row"][4:]
        assert (rec["via"] == "gen_kernel") == (tuple(rec["params"]) == cs.REF_CLICKS)
    assert any(tuple(r[0]["params"]) != cs.REF_CLICKS for r in recs.values())

    def picks_by_rank(key):
        rec, obj, box, pts, cnt, trace = recs[key]
        out = [tuple(p) for p in pts[0, :cnt[0]] if not trace["fg"]["small"]]
        n_bg = cnt[1] if key[1] == 1 else min(cnt[1], 1)
        return out + [tuple(p) for p in pts[1, :n_bg] if not trace["bg"]["small"]], box

    # a rank pick in a slice other than the first, and one past the first trip of the selecting loop in its slice
    later_slice = past_trip = 0
    for key in recs:
        picked, box = picks_by_rank(key)
        chunk = c3.chunk_of(box[3] * box[4])
        later_slice += sum(1 for z, y, x in picked if z > 0)
        past_trip += sum(1 for z, y, x in picked if (y * box[4] + x) % chunk >= c3.TRIP)
    assert later_slice > 0 and past_trip > 0
    # strategy 3: a winner that the in-plane distance alone would not pick, and a tie across two slices
    assert recs[("sym", 3)][5]["bg"]["dz_wins"] > 0 and recs[("sym", 3)][5]["bg"]["cross_ties"] > 0
    assert recs[("sym", 3)][3][1, 1, 0] == 0                                         # ... resolved for the first slice
    # a later click within `step` in the plane of an earlier one, on another slice: suppression does not leak
    rec, _, _, pts, cnt, _ = recs[("multi", 1)]
    (z0, y0, x0), (z1, y1, x1) = pts[0, 0], pts[0, 1]
    assert z0 != z1 and (y0 - y1) ** 2 + (x0 - x1) ** 2 <= rec["params"][1] ** 2
    # a kind that stops because nothing is left, with clicks on several slices
    _, _, _, pts, cnt, trace = recs[("stop", 1)]
    assert trace["fg"]["emptied"] and cnt[0] == 3 and len(set(pts[0, :3, 0].tolist())) == 3
    # "small" with a mean at .5: (is half, floor & 1) per axis (z, y, x)
    assert recs[("tiny_a", 1)][5]["fg"]["small"] and recs[("tiny_a", 1)][5]["fg"]["half"] == [(True, 1), (False, 0), (True, 0)]
    assert recs[("tiny_b", 1)][5]["fg"]["small"] and recs[("tiny_b", 1)][5]["fg"]["half"] == [(True, 0), (False, 0), (True, 1)]
    assert recs[("tiny_a", 1)][3][0, 0].tolist() == [2, 10, 10] and recs[("tiny_b", 1)][3][0, 0].tolist() == [0, 10, 12]
    # a crop clamped into the far (y, x) corner
    rec, _, box, _, _, _ = recs[("multi", 1)]
    vol = c3.build(rec["volume"])
    assert box[1] + box[3] == vol.shape[1] and box[2] + box[4] == vol.shape[2]
    assert rec["centre"][1] - rec["crop"][0] // 2 > box[1] and rec["centre"][2] - rec["crop"][1] // 2 > box[2]
    # a case shallower than D, no object, all object
    rec, obj, _, _, _, _ = recs[("shallow", 1)]
    assert c3.build(rec["volume"]).shape[0] == 4 and rec["depth"] == 6 and not obj[4:].any() and obj[:4].any()
    _, obj, _, _, cnt, trace = recs[("none", 1)]
    assert not obj.any() and cnt.tolist() == [0, 1] and trace["bg"]["small"]
    _, obj, _, _, cnt, _ = recs[("all", 3)]
    assert obj.all() and cnt.tolist() == [4, 0]


# ------------------------------------------------------------------------------------------------- the library
def _desc(n=4, d=10, h=256, w=256, n_slices=1000, src=(512, 512), clicks=(3, 10, 40, 5), g=2, gaussian=1, stddev=(1, 3, 3),
          norm=1.0):
    from boxsegliver_amd import _abi
    return _abi.Lits3dClicksDesc(N=n, D=d, H=h, W=w, n_slices=n_slices, src_h=src[0], src_w=src[1], lab_scale=64, obj_label=2,
                                 margin=clicks[0], step=clicks[1], band=clicks[2], max_clicks=clicks[3], G=g, gaussian=gaussian,
                                 stddev=(ctypes.c_float * 3)(*stddev), euclid_norm=norm)


def test_the_library_exports_the_new_entry_points_and_checks_their_arguments():
    """Every refusal returns before anything is launched."""
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_lits3d_clicks_ws_bytes", "unetk_lits3d_clicks", "unetk_click_guide3d"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.unetk_abi_version() == 10                                             # additive
    d = _desc()
    nbytes = lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(d))
    assert nbytes == 4 * 3 * 10 * 512 * 512 + 4 * 10 * 512 * 32 and nbytes % 16 == 0   # three byte fields + the row records
    odd = _desc(n=1, d=3, src=(7, 9))
    assert lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(odd)) == 3 * 192 + 3 * 7 * 32  # 3 * 63 voxels -> 192 per field
    p = ctypes.c_void_p(1 << 20)                                                     # never dereferenced: the calls return first
    assert lib.unetk_lits3d_clicks(ctypes.byref(d), p, p, p, p, p, p, p, nbytes - 1, None) == -3      # UNETK_E_WORKSPACE
    assert lib.unetk_lits3d_clicks(ctypes.byref(d), p, p, p, None, p, p, p, nbytes, None) == -1       # UNETK_E_BADARG
    assert lib.unetk_lits3d_clicks(ctypes.byref(d), p, p, p, p, p, p, ctypes.c_void_p((1 << 20) + 8), nbytes, None) == -1
    assert lib.unetk_lits3d_clicks(ctypes.byref(d), p, p, ctypes.c_void_p((1 << 20) + 2), p, p, p, p, nbytes, None) == -1
    for bad in (_desc(clicks=(0, 10, 40, 5)), _desc(clicks=(3, 10, 0, 5)), _desc(clicks=(3, -1, 40, 5)), _desc(clicks=(3, 10, 252, 5)),
                _desc(clicks=(3, 10, 40, 6)), _desc(clicks=(3, 10, 40, 1)), _desc(src=(1025, 512)), _desc(src=(512, 1025)),
                _desc(d=257), _desc(d=257, n=1)):
        assert lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.unetk_lits3d_clicks(ctypes.byref(bad), p, p, p, p, p, p, p, 1 << 30, None) == -2   # UNETK_E_UNSUPPORTED
    assert lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(_desc(clicks=(3, 10, 251, 5)))) > 0          # margin + band = 254
    assert lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(_desc(d=256, n=1))) > 0
    for bad in (_desc(n=0), _desc(d=0), _desc(n=65536), _desc(n_slices=0)):
        assert lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.unetk_lits3d_clicks(ctypes.byref(bad), p, p, p, p, p, p, p, 1 << 30, None) == -1
    # the guide
    assert lib.unetk_click_guide3d(ctypes.byref(d), p, p, p, None, None) == -1
    assert lib.unetk_click_guide3d(ctypes.byref(d), p, p, p, ctypes.c_void_p((1 << 20) + 2), None) == -1
    assert lib.unetk_click_guide3d(ctypes.byref(_desc(g=3)), p, p, p, p, None) == -1
    assert lib.unetk_click_guide3d(ctypes.byref(_desc(stddev=(1, 0, 3))), p, p, p, p, None) == -1
    assert lib.unetk_click_guide3d(ctypes.byref(_desc(gaussian=0, norm=0.0)), p, p, p, p, None) == -1
    assert lib.unetk_click_guide3d(ctypes.byref(_desc(n=1, d=2048, h=1024, w=1024)), p, p, p, p, None) == -2   # D*H*W = 2^31
    # the 2-D entry points are still there
    for name in ("unetk_lits_clicks", "unetk_click_guide", "unetk_lits_patch3d"):
        assert hasattr(lib, name)


# ------------------------------------------------------------------------------------------------- the sampler stream
class _FakeStore(object):
    device = torch.device("cpu")

    def __init__(self):
        self.im = torch.zeros((sum(ref.DEPTHS), ref.H, ref.W), dtype=torch.int16)
        self.lb = torch.zeros((sum(ref.DEPTHS), ref.H, ref.W), dtype=torch.uint8)


def _stream(monkeypatch, guide, n=6):
    """The sample tables (and click tables) `lits3d.batches` uploads, with the device calls replaced by recorders."""
    from boxsegliver_amd.data import lits, lits3d
    from test_lits3d_host import _sampler
    sampler, _, _ = _sampler(bs=2, tumor_percent=0.5, seed=1234, random_flip=7)
    tabs, ctabs = [], []

    def upload(parts, device):
        tabs.append(parts[0].copy())
        if len(parts) > 1:
            ctabs.append(parts[1].copy())
        return [torch.from_numpy(p.copy()) for p in parts]
    shape = (6, 16, 20)
    monkeypatch.setattr(lits, "upload_pinned", upload)
    monkeypatch.setattr(lits3d.ops, "lits_pick_voxels", lambda *a, **k: None)
    monkeypatch.setattr(lits3d.ops, "lits_patch3d", lambda *a, **k: (torch.zeros(1), torch.zeros(1)))
    monkeypatch.setattr(lits3d.ops, "lits3d_clicks", lambda *a, **k: (torch.zeros(1), torch.zeros(1)))
    monkeypatch.setattr(lits3d.ops, "click_guide3d", lambda *a, **k: torch.zeros(1))
    gen = lits3d.batches(_FakeStore(), sampler, shape, 2, 2, torch.zeros(1, dtype=torch.int32), guide)
    feats = [next(gen)[0] for _ in range(n)]
    return np.stack(tabs), ctabs, feats


def test_an_unguided_stream_consumes_the_generator_as_before(monkeypatch):
    from test_lits3d_host import _sampler
    plain, ctabs, feats = _stream(monkeypatch, None)
    assert ctabs == [] and all("sp_guide" not in f for f in feats)
    sampler, _, _ = _sampler(bs=2, tumor_percent=0.5, seed=1234, random_flip=7)
    np.testing.assert_array_equal(plain, np.stack([sampler.table() for _ in range(6)]))     # nothing but the sampler's draws
    guided, ctabs, feats = _stream(monkeypatch, dict(channels=2, stddev=None))
    assert len(ctabs) == 6 and all("sp_guide" in f for f in feats)
    np.testing.assert_array_equal(guided[0], plain[0])                                # the click draws come after the sampler's
    assert not np.array_equal(guided[1:], plain[1:])
    for c in ctabs:
        c = c.view(np.uint32)
        assert c.shape == (2, 12) and np.all((c[:, 0] >= 1) & (c[:, 0] < 5)) and np.all(c[:, 1] < 5) and set(c[:, 2]) <= {1, 3}
