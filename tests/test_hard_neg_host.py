"""CPU: hard-negative training of `liver_3d` -- the flags and their refusals, `PatchSampler.draw_hard_neg`,
the neg-<PID>.npz round trip, and the restatements the GPU tests lean on (hard_neg_ref.py): the mining rule on hand-made
volumes and the strategy-4 click loop against what the reference itself gave (tests/golden/ref_clicks3d_neg.json)."""
import json
import math
import os

import numpy as np
import pytest

import click3d_shapes as c3
import hard_neg_ref as hn
import lits3d_clicks_ref as cref
import lits3d_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = "liver_3d --mode train --tag t --model UNet3D --classes Liver Tumor --batch_size 4 --tumor_percent 0.5"


def _args(extra="", base=BASE):
    from boxsegliver_amd.entry import main as entry
    return entry.get_arguments((base + " " + extra).split())[0]


# ------------------------------------------------------------------------------------------------- flags
def test_flags_parse_with_their_defaults():
    from boxsegliver_amd.data import lits3d
    a = _args()
    assert a.hard_neg_from is None and a.hard_neg_patches == 0.0 and a.hard_neg_clicks is False
    assert lits3d.hard_negatives(a) is None and lits3d.check_args(a) == (2, 2)
    a = _args("--hard_neg_from /x/neg3d --hard_neg_patches 0.25 --hard_neg_clicks --use_spatial")
    assert lits3d.check_args(a) == (2, 2)
    hard = lits3d.hard_negatives(a)
    assert (hard["directory"], hard["patches"], hard["clicks"]) == ("/x/neg3d", 0.25, True)
    a = _args("--hard_neg_from /x/neg3d --hard_neg_patches 0.5")                      # patches work without --use_spatial
    assert lits3d.hard_negatives(a)["clicks"] is False and lits3d.check_args(a) == (2, 2)


@pytest.mark.parametrize("extra,name", [
    ("--hard_neg_patches 0.25", "--hard_neg_patches"),                               # a training flag without the directory
    ("--hard_neg_clicks --use_spatial", "--hard_neg_clicks"),
    ("--hard_neg_from /x", "--hard_neg_from"),                                       # the directory without a training flag
    ("--hard_neg_from /x --hard_neg_patches 0", "--hard_neg_from"),
    ("--hard_neg_from /x --hard_neg_clicks", "--hard_neg_clicks"),                   # clicks without --use_spatial
    ("--hard_neg_from /x --hard_neg_patches 1.5", "--hard_neg_patches"),
    ("--hard_neg_from /x --hard_neg_patches -0.1", "--hard_neg_patches"),
    ("--hard_neg_from /x --hard_neg_patches nan", "--hard_neg_patches"),
    ("--hard_neg_from /x --hard_neg_patches 0.75", "--hard_neg_patches"),            # ceil(4 * 0.5) + ceil(4 * 0.75) > 4
    ("--hard_neg_from /x --hard_neg_patches 0.51", "--hard_neg_patches"),            # 2 + 3 > 4
])
def test_refusals_name_the_flag(extra, name):
    from boxsegliver_amd.data import lits3d
    a = _args(extra)
    with pytest.raises(ValueError, match=name):
        lits3d.check_args(a)
    with pytest.raises(ValueError, match=name):                                      # before anything is loaded: no root exists
        lits3d.input_fn("train", {"args": a, "lits_root": "/nonexistent"})


@pytest.mark.parametrize("mode", ["eval", "infer"])
@pytest.mark.parametrize("extra,name", [("--hard_neg_from /x --hard_neg_patches 0.25", "--hard_neg_from"),
                                        ("--hard_neg_from /x --hard_neg_patches 0.25", "--hard_neg_patches"),
                                        ("--hard_neg_from /x --hard_neg_clicks --use_spatial", "--hard_neg_clicks")])
def test_the_flags_serve_training_only(mode, extra, name):
    from boxsegliver_amd.data import lits3d
    a = _args(extra + " --eval_in_patches", BASE.replace("--mode train", "--mode " + mode))
    with pytest.raises(ValueError, match=name):
        lits3d.check_args(a)


@pytest.mark.parametrize("flag", ["--fp_sample", "--sample_neg 0.25"])
def test_the_reference_names_stay_rejected(flag, capsys):
    with pytest.raises(SystemExit):
        _args(flag)
    assert flag.split()[0] in capsys.readouterr().err


def test_the_largest_share_that_fits_is_accepted():
    from boxsegliver_amd.data import lits3d
    assert lits3d.hard_negatives(_args("--hard_neg_from /x --hard_neg_patches 0.5"))["patches"] == 0.5      # 2 + 2 == 4
    assert lits3d.hard_negatives(_args("--hard_neg_from /x --hard_neg_patches 1.0 --tumor_percent 0"))["patches"] == 1.0


# ------------------------------------------------------------------------------------------------- sampler
def _sampler(bs=4, tumor_percent=0.5, patches=0.25, seed=7, training=True, fg=2, neg=None):
    from boxsegliver_amd.data import lits3d
    cases = ref.make_cases()
    _, lb, base = ref.stack_store(cases)
    counts = (lb // 64 >= fg).sum(axis=(1, 2))
    neg = hn.store_neg() if neg is None else neg
    neg_counts = np.concatenate([n.sum(axis=(1, 2)) for n in neg]).astype(np.int64)
    meta = [{"PID": pid, "size": [im.shape[0], ref.H, ref.W]} for pid, (im, _) in enumerate(cases)]
    offset = {pid: int(b) for pid, b in enumerate(base)}
    s = lits3d.PatchSampler(meta, offset, counts, bs, (6, 16, 20), (ref.H, ref.W), tumor_percent=tumor_percent, training=training,
                            seed=seed, hard_neg_patches=patches, neg_counts=neg_counts)
    return s, cases, neg, base


@pytest.mark.parametrize("bs,tp,p", [(4, 0.5, 0.25), (4, 0.5, 0.5), (3, 0.0, 1.0), (4, 0.25, 0.3)])
def test_draw_hard_neg_rows_cases_and_centres(bs, tp, p):
    from boxsegliver_amd.data import lits3d
    s, cases, neg, base = _sampler(bs, tp, p)
    force, force_fp = int(math.ceil(bs * tp)), int(math.ceil(bs * p))
    assert (s.force, s.force_fp) == (force, force_fp)
    fg_cases = {0, 2, 3}                                                              # the cases that hold a tumour
    seen = {"neg": 0, "uniform": 0}
    for _ in range(60):
        b = s.draw_hard_neg(s.draw())
        rows = range(force, force + force_fp)
        picked = [int(b["case"][j]) for j in rows]
        assert set(picked) <= fg_cases and len(set(picked)) == force_fp               # from fg_cases, without replacement
        assert b["forced"][:force].tolist() == [lits3d.FORCED_LABEL] * force
        assert not b["forced"][force + force_fp:].any()
        tab = s.table(b)
        np.testing.assert_array_equal(tab[:, lits3d.COL_FORCED], b["forced"])
        np.testing.assert_array_equal(tab[:, lits3d.COL_BASE], base[b["case"]])
        np.testing.assert_array_equal(b["pid"], b["case"])
        for j in rows:
            ci, (z, y, x) = picked[j - force], b["center"][j]
            assert 0 <= z < ref.DEPTHS[ci]
            if neg[ci].any():
                assert b["forced"][j] == lits3d.FORCED_NEG and 0 <= b["k"][j] < neg[ci][z].sum() and (y, x) == (0, 0)
                seen["neg"] += 1
            else:                                                                     # case 2: a uniform centre in its own extents
                assert b["forced"][j] == 0 and b["k"][j] == 0 and 0 <= y < ref.H and 0 <= x < ref.W
                seen["uniform"] += 1
    assert seen["neg"] > 0 and seen["uniform"] > 0


def test_locate_neg_equals_the_restatement_at_the_slice_boundaries():
    s, _, neg, _ = _sampler()
    for ci, mask in enumerate(neg):
        total = int(mask.sum())
        assert s.neg_total[ci] == total
        if total == 0:
            continue
        per_slice = mask.sum(axis=(1, 2))
        edges = np.cumsum(per_slice[per_slice > 0])[:-1]                              # first ranks of the later slices
        ranks = sorted({0, total - 1} | {int(e) - 1 for e in edges} | {int(e) for e in edges})
        z, k = s.locate_neg(np.full(len(ranks), ci), ranks)
        pos = np.argwhere(mask)
        for r, zz, kk in zip(ranks, z, k):
            assert (int(zz), int(kk)) == hn.locate(mask, r)
            np.testing.assert_array_equal(np.argwhere(mask[zz])[kk], pos[r, 1:])
    assert len(edges) > 0


def test_a_sampler_without_the_flag_draws_as_before():
    from boxsegliver_amd.data import lits3d
    plain, cases, _, base = _sampler(patches=0.0)
    _, lb, _ = ref.stack_store(cases)
    meta = [{"PID": pid, "size": [im.shape[0], ref.H, ref.W]} for pid, (im, _) in enumerate(cases)]
    parent = lits3d.PatchSampler(meta, {pid: int(b) for pid, b in enumerate(base)}, (lb // 64 >= 2).sum(axis=(1, 2)), 4, (6, 16, 20),
                                 (ref.H, ref.W), tumor_percent=0.5, training=True, seed=7)           # constructed as the parent does
    assert plain.force_fp == 0 and parent.force_fp == 0
    for _ in range(5):
        a, b = plain.draw_hard_neg(plain.draw()), parent.draw()
        assert a.keys() == b.keys()
        for key in a:
            np.testing.assert_array_equal(a[key], b[key])
        np.testing.assert_array_equal(plain.table(a), parent.table(b))
    assert plain.rng.bit_generator.state == parent.rng.bit_generator.state
    # evaluation never re-targets a row, whatever the share
    ev, _, _, _ = _sampler(patches=0.5, training=False)
    assert ev.force_fp == 0
    # the flagged sampler makes its extra draws after `draw`: the first batch's own draw is the unflagged one
    flagged, _, _, _ = _sampler(patches=0.25)
    fresh, _, _, _ = _sampler(patches=0.0)
    a, b = flagged.draw(), fresh.draw()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key])


def test_sampler_refuses_more_forced_rows_than_the_batch_has():
    with pytest.raises(ValueError, match="--hard_neg_patches"):
        _sampler(bs=4, tumor_percent=0.5, patches=0.75)
    with pytest.raises(ValueError, match="--hard_neg_patches"):                       # 4 rows without replacement from 3 cases
        _sampler(bs=4, tumor_percent=0.0, patches=1.0)


# ------------------------------------------------------------------------------------------------- files
def test_npz_round_trip(tmp_path):
    from boxsegliver_amd.data import extract
    mask = hn.store_neg()[0]
    path = tmp_path / "neg-0.npz"
    extract.save_neg(path, mask * 7, mask.sum(axis=(1, 2)), 3, 5)                     # any non-zero value is a voxel
    rec = extract.load_neg(path)
    assert rec["shape"] == mask.shape and rec["kept"] == 3 and rec["components"] == 5
    assert rec["slice_counts"].dtype == np.int64 and rec["slice_counts"].tolist() == mask.sum(axis=(1, 2)).tolist()
    np.testing.assert_array_equal(rec["bits"], np.packbits(mask.reshape(-1)))
    np.testing.assert_array_equal(extract.unpack_neg(rec), mask)
    odd = np.zeros((3, 5, 7), np.uint8)                                               # 105 voxels: the last byte is padded
    odd[2, 4, 6] = odd[0, 0, 0] = 1
    extract.save_neg(tmp_path / "odd.npz", odd, odd.sum(axis=(1, 2)), 2, 2)
    np.testing.assert_array_equal(extract.unpack_neg(extract.load_neg(tmp_path / "odd.npz")), odd)
    np.savez(tmp_path / "bad.npz", bits=np.zeros(3, np.uint8), shape=np.array([3, 5, 7]), slice_counts=np.zeros(3, np.int64),
             kept=0, components=0)
    with pytest.raises(ValueError, match="bad.npz"):
        extract.load_neg(tmp_path / "bad.npz")
    np.savez(tmp_path / "other.npz", mask=odd)
    with pytest.raises(ValueError, match="other.npz"):
        extract.load_neg(tmp_path / "other.npz")


# ------------------------------------------------------------------------------------------------- the mining rule
def test_mining_restatement_on_hand_made_volumes():
    pred = np.zeros((4, 8, 10), np.uint8)
    lab = np.zeros_like(pred)
    pred[0, 0, 0:6] = 2                      # 6 voxels in a row: kept at min_size 6
    pred[1, 3, 0:5] = 2                      # 5 voxels: dropped at 6, kept at 5
    pred[2, 0:3, 8:10] = 2                   # 6 voxels, one of them on the labelled object: dropped
    lab[2, 2, 9] = 2
    pred[3, 5:8, 2:4] = 1                    # liver-valued prediction: not part of the tumour object, and not an overlap
    pred[0:3, 7, 5] = 2                      # spans slices with ...
    pred[2, 7, 6:9] = 2                      # ... an L: 6 voxels
    lab[3, 6, 2] = 1                         # labelled LIVER under nothing predicted as tumour
    out, counts, head = hn.fp_mask(pred, lab, 2, 2, 6)
    assert head == [4, 2, 12, 0] and counts.tolist() == [7, 1, 4, 0]
    assert out[0, 0, :6].all() and out[0:3, 7, 5].all() and out[2, 7, 6:9].all() and out.sum() == 12
    assert hn.fp_mask(pred, lab, 2, 2, 5)[2] == [4, 3, 17, 0]
    # the overlap is tested against the object class: a predicted tumour inside labelled LIVER is a false positive ...
    lab2 = lab.copy()
    lab2[0, 0, 0:6] = 1
    assert hn.fp_mask(pred, lab2, 2, 2, 6)[2] == [4, 2, 12, 0]
    # ... and with the liver as the object (--classes Liver) it is not; the liver-valued block now counts, and lies on labelled
    # liver: of the five components only the L is kept
    out1, _, head1 = hn.fp_mask(pred, lab2, 1, 1, 6, out_value=64)
    assert head1 == [5, 1, 6, 0] and set(np.unique(out1).tolist()) == {0, 64} and not out1[0, 0, 0:6].any()
    assert out1[0:3, 7, 5].all() and out1[2, 7, 6:9].all()
    # two blobs that touch only diagonally are two components; the end of a row does not touch the start of the next
    p = np.zeros((1, 4, 6), np.uint8)
    p[0, 0, 0] = p[0, 1, 1] = p[0, 2, 5] = p[0, 3, 0] = 1
    assert hn.fp_mask(p, np.zeros_like(p), 1, 1, 1)[2] == [4, 4, 4, 0]
    assert hn.fp_mask(np.zeros_like(p), np.zeros_like(p), 1, 1, 1)[2] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- clicks: the records
def _fixture():
    with open(os.path.join(HERE, "golden", "ref_clicks3d_neg.json")) as f:
        return json.load(f)


def test_click_restatement_equals_the_reference_records():
    fixture = _fixture()
    for name, want in fixture["masks"].items():
        assert c3.checksum(hn.build_neg(name)) == (want["popcount"], want["index_sum"]) and hn.NEG_MASKS[name][0] == want["volume"]
    assert [(r[0], row) for r in hn.RECORDS for row in r[6]] == [(r["id"], r["row"]) for r in fixture["records"]]
    with open(os.path.join(HERE, "golden", "ref_clicks3d.json")) as f:
        plain = {(r["id"], tuple(r["row"])): r for r in json.load(f)["records"]}
    seen = dict(one=0, many=0, stopped=0, none_asked=0, beyond=0, outside=0, label=0)
    for rec in fixture["records"]:
        vol, neg = c3.build(rec["volume"]), hn.build_neg(rec["neg"])
        shape, crop, params = (rec["depth"],) + tuple(rec["crop"]), tuple(rec["crop"]), tuple(rec["params"])
        obj, box = cref.object_patch(vol, rec["centre"], crop, shape, 1)
        assert [box[0], box[1], box[2]] == rec["box"][:3]
        patch = hn.neg_patch(neg, rec["centre"], crop, shape)
        assert int(patch.sum()) == rec["neg_in_patch"]
        trace = {}
        pts, cnt = hn.clicks(obj, patch, np.array(rec["row"], np.uint64), params, trace)
        assert pts[0, :cnt[0]].tolist() == rec["fg"] and pts[1, :cnt[1]].tolist() == rec["bg"], rec["id"]
        assert [list(v) for v in zip(trace["bg"].get("ranks", []), trace["bg"].get("counts", []))] == rec["asked"]["bg"]
        if rec["same_as"]:                                                            # no false positive in the crop: the plain record
            same = plain[(rec["same_as"], tuple(rec["row"]))]
            assert rec["neg_in_patch"] == 0 and (rec["fg"], rec["bg"]) == (same["fg"], same["bg"])
            seen["beyond" if rec["box_via"] == "padded" else "outside"] += 1
            continue
        assert rec["neg_in_patch"] > 0
        for z, y, x in rec["bg"]:                                                     # every background click is a false positive
            assert patch[z, y, x] == 1
            seen["label"] += int(obj[z, y, x] == 1)                                   # ... whatever the label says there
        slices = {p[0] for p in rec["bg"]}
        seen["one"] += int(len(rec["bg"]) == 4 and len(slices) == 1)
        seen["many"] += int(len(slices) > 1)
        seen["stopped"] += int(0 < len(rec["bg"]) < rec["row"][1])
        seen["none_asked"] += int(rec["row"][1] == 0 and rec["bg"] == [])
        if rec["id"] == "several":                                                    # ranks cross slices: (z, y, x) order
            assert rec["asked"]["bg"][0][0] == rec["asked"]["bg"][0][1] - 1 and rec["asked"]["bg"][1][0] == 0
            assert rec["bg"][0][0] == max(slices) and rec["bg"][1][0] == min(slices)
        # the strategy column is not used: both rows of a record give the same clicks
    assert all(v > 0 for v in seen.values()), seen
    by_id = {}
    for rec in fixture["records"]:
        by_id.setdefault(rec["id"], []).append(rec["bg"])
    assert all(a == b for rid, (a, b) in by_id.items() if rid not in ("shallow", "outside"))
