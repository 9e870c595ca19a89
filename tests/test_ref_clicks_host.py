"""CPU: the click records of tests/golden/ref_clicks.json -- what the reference's img_crop, gen_kernel and inter_simulation
gave on the label slices of click_shapes.py (tests/golden/make_click_fixtures.py) -- against the restatement the other click
tests hang from (lits_inter_ref.clicks, lits_inter_ref.crop_box), and the conditions that make the records worth their
place: every loop of clk_select_kernel, clk_rows_kernel and clk_cols_kernel repeats on them."""
import json
import os

import numpy as np
import pytest
from scipy.ndimage import distance_transform_cdt

import click_shapes as cs
import lits_inter_ref as ref

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_clicks.json")) as _f:
    FIXTURE = json.load(_f)
RECORDS = FIXTURE["records"]
IDS = [s[0] for s in cs.SHAPES]


@pytest.fixture(scope="module")
def masks():
    out = {}
    for name, (shape, ellipses, rects) in cs.MASKS.items():
        m = cs.build(shape, ellipses, rects)
        want = FIXTURE["masks"][name]
        assert list(m.shape) == want["shape"] and cs.checksum(m) == (want["popcount"], want["index_sum"]), name
        out[name] = m
    assert set(out) == set(FIXTURE["masks"])
    return out


def _crop(masks, rec):
    y1, y2, x1, x2 = rec["slices"]
    return masks[rec["mask"]][y1:y2, x1:x2]


def _restated(masks, rec):
    tr = {}
    pts, cnt = ref.clicks(_crop(masks, rec), np.array(rec["row"], np.uint64), tuple(rec["params"]), tr)
    return pts, cnt, tr


def test_fixture_lists_the_shapes_of_click_shapes():
    want = [(sid, mask, list(centre), list(crop), list(params), list(row))
            for sid, mask, centre, crop, params, rows in cs.SHAPES for row in rows]
    got = [(r["id"], r["mask"], r["centre"], r["crop"], r["params"], r["row"]) for r in RECORDS]
    assert got == want
    for r in RECORDS:
        assert r["via"] == ("gen_kernel" if tuple(r["params"]) == cs.REF_CLICKS else "inter_simulation")
        assert bool(r["raises"]) == (r["id"] == "wide_all")                    # the one documented deviation
    assert cs.rank_draw(5, 12) * 12 >> 32 == 5 and cs.rank_draw(0, 7) == 0 and (cs.LAST * 9600) >> 32 == 9599


def test_restated_crop_box_equals_the_reference_slices(masks):
    for r in RECORDS:
        y1, x1, ch, cw = ref.crop_box(r["centre"], r["crop"], masks[r["mask"]].shape)
        assert [y1, y1 + ch, x1, x1 + cw] == r["slices"], r["id"]


@pytest.mark.parametrize("sid", IDS)
def test_restated_clicks_equal_the_reference(masks, sid):
    recs = [r for r in RECORDS if r["id"] == sid]
    assert len(recs) == 2
    for r in recs:
        pts, cnt, tr = _restated(masks, r)
        for kind, name in enumerate(("fg", "bg")):
            assert cnt[kind] == len(r[name]), (sid, name)
            assert pts[kind, :cnt[kind]].tolist() == r[name], (sid, name)
            assert np.all(pts[kind, cnt[kind]:] == -1)
            if r[name] or not r["raises"]:                                     # every (rank, count) the reference drew
                asked = [list(a) for a in zip(tr[name].get("ranks", []), tr[name].get("counts", []))]
                assert asked == r["asked"][name], (sid, name)


# ------------------------------------------------------------------------------------------------- what the records hold
def _picks(masks, sid):
    """(random-rank picks, strategy-3 arg-max picks) of a shape's records as flat crop indices, from the restatement's trace
    and the recorded clicks: click k is a rank pick when k == 0 or the strategy is 1, an arg-max otherwise; a "small" mask
    has neither."""
    rank, argmax = [], []
    for r in (r for r in RECORDS if r["id"] == sid):
        _, _, tr = _restated(masks, r)
        cw = r["slices"][3] - r["slices"][2]
        for name, strategy in (("fg", 1), ("bg", r["row"][2])):
            if not r[name] or tr[name]["small"]:
                continue
            for k, (y, x) in enumerate(r[name]):
                (rank if k == 0 or strategy == 1 else argmax).append(y * cw + x)
    return rank, argmax


LOOPED = ["two_trips", "wide", "wide_cap255", "wide_small", "row_limit", "col_limit", "full", "full_tiny", "wide_all"]


@pytest.mark.parametrize("sid", LOOPED)
def test_picks_lie_past_the_first_trip_and_in_the_first_and_last_wave(masks, sid):
    rec = [r for r in RECORDS if r["id"] == sid][0]
    total = (rec["slices"][1] - rec["slices"][0]) * (rec["slices"][3] - rec["slices"][2])
    chunk = cs.chunk_of(total)
    assert chunk > cs.TRIP
    last_wave = (total - 1) // chunk
    rank, argmax = _picks(masks, sid)
    assert any(i % chunk >= cs.TRIP for i in rank)                             # the `rank -= here` carry across trips
    assert any(i // chunk == 0 for i in rank)
    assert any(i // chunk == last_wave for i in rank)
    if sid != "wide_all":                                                      # an all-object crop has no background click
        assert any(i % chunk >= cs.TRIP for i in argmax)
    if sid == "two_trips":
        assert total % cs.TRIP != 0 and chunk % cs.TRIP != 0 and chunk // cs.TRIP == 1      # one full trip and a ragged one
        assert last_wave == 14                                                 # the sixteenth wave has no pixel


def test_the_other_shapes_have_no_candidate_picks(masks):
    assert sorted(set(IDS) - set(LOOPED)) == ["wide_none"]
    assert _picks(masks, "wide_none") == ([], [])
    a, b = [r for r in RECORDS if r["id"] == "wide_none"]
    assert a["row"][1] == 0 and a["bg"] == [] and b["row"][1] == 1 and b["bg"] == [[64, 149]] and a["fg"] == b["fg"] == []
    for r in (r for r in RECORDS if r["id"] == "wide_all"):
        assert _crop(masks, r).min() == 1 and r["bg"] == [] and len(r["fg"]) == 4
    for r in (r for r in RECORDS if r["id"] == "full_tiny"):
        _, _, tr = _restated(masks, r)
        assert tr["fg"]["small"] and len(r["fg"]) == 1 and not tr["bg"]["small"] and not tr["bg"]["band_cut"]
        ys = np.nonzero(_crop(masks, r))[0]
        chunk_rows = cs.chunk_of(1024 * 1024) // 1024
        assert len(set((ys // chunk_rows).tolist())) == 3                      # the mean's terms come from three waves


def _taxicab(zero):
    """City-block distance of every pixel to the nearest True pixel of `zero` (a large value where there is none)."""
    if not zero.any():
        return np.full(zero.shape, 1 << 20, np.int64)
    return distance_transform_cdt(~zero, metric="taxicab").astype(np.int64)


@pytest.mark.parametrize("sid", ["wide", "wide_cap255", "wide_small"])
def test_wide_rows_need_the_second_pixel_of_a_row_thread(masks, sid):
    rec = [r for r in RECORDS if r["id"] == sid][0]
    obj = _crop(masks, rec).astype(bool)
    margin, _, band, _ = rec["params"]
    assert obj.shape == (130, 300)
    crossing = 0
    for bg in (False, True):
        mask = ~obj if bg else obj
        cand = ref.candidates(mask, margin, band, bg)
        assert cand[:, 256:].any() and cand[:, 64:256].any()                   # five column blocks, two pixels per row thread
        left, right = mask.copy(), mask.copy()
        left[:, 256:] = True                                                   # zeros at x < 256 only
        right[:, :256] = True
        d_left, d_right = _taxicab(~left), _taxicab(~right)
        border = np.full(obj.shape, 1 << 20, np.int64)
        if not bg:                                                             # the crop's border is a zero of the foreground
            yy, xx = np.mgrid[:130, :300]
            border = np.minimum(np.minimum(yy + 1, 130 - yy), np.minimum(xx + 1, 300 - xx))
        crossing += int((cand[:, :256] & (d_right[:, :256] < np.minimum(d_left, border)[:, :256])).sum())
        crossing += int((cand[:, 256:] & (d_left[:, 256:] < np.minimum(d_right, border)[:, 256:])).sum())
    assert crossing > 0                                                        # a nearest zero on the other side of x = 256


def test_far_pixels_clamp_and_cap(masks):
    for sid in ("full_tiny", "wide"):
        rec = [r for r in RECORDS if r["id"] == sid][0]
        obj = _crop(masks, rec).astype(bool)
        assert (_taxicab(obj)[~obj] > rec["params"][0] + rec["params"][2]).any(), sid      # beyond the band's outer edge
    rec = [r for r in RECORDS if r["id"] == "two_trips"][0]
    assert [rec["centre"][0] - rec["crop"][0] // 2, rec["centre"][1] - rec["crop"][1] // 2] != [rec["slices"][0], rec["slices"][2]]
    assert rec["slices"] == [4, 100, 4, 104] and masks[rec["mask"]].shape == (100, 104)    # clamped into the far corner
    rec = [r for r in RECORDS if r["id"] == "wide_cap255"][0]
    obj = _crop(masks, rec).astype(bool)
    cap = rec["params"][0] + rec["params"][2] + 1
    d = _taxicab(obj)
    assert cap == 255 and (np.minimum(d, cap) == 255).any() and (d == 254).any()           # 255 in the byte fields, next to 254
    # pixels inside the band whose nearest object column is 128 or more columns away: the last doubling step decides them
    cols = np.flatnonzero(obj.any(axis=0))
    far = np.abs(np.arange(300)[:, None] - cols[None, :]).min(axis=1) >= 128
    assert (d[:, far] <= cap - 1).any()
