"""Host: the window plan of the sliding-window UNet3D evaluation (data/lits3d.py: window_starts, eval_tables, the flags;
DESIGN.md 7.3.4) and the float64 restatement of the accumulate step the GPU tests compare with (eval3d_ref.py)."""
import numpy as np
import pytest

import eval3d_ref
import lits3d_ref as ref

SMALL = (6, 16, 20)
EVAL_ARGV = ("liver_3d --mode eval --tag t --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 6 --im_height 16 "
             "--im_width 20 --batch_size 5 --evaluator Volume --eval_in_patches").split()


@pytest.mark.parametrize("extent,window,overlap", [(12, 6, 0.5), (40, 18, 0.5), (48, 22, 0.5), (9, 6, 0.5), (41, 10, 0.0),
                                                   (40, 10, 0.0), (100, 7, 0.9), (30, 7, 0.99), (512, 288, 0.5), (7, 6, 0.5)])
def test_window_starts_cover_the_axis(extent, window, overlap):
    from boxsegliver_amd.data import lits3d
    starts = lits3d.window_starts(extent, window, overlap)
    step = max(int(window * (1 - overlap)), 1)
    assert starts[0] == 0 and starts == sorted(set(starts))
    assert starts[-1] + window == extent                                             # the last window ends at the end
    covered = np.zeros(extent, bool)
    for a in starts:
        assert 0 <= a and a + window <= extent
        covered[a:a + window] = True
    assert covered.all()
    regular = [a for a in starts if a % step == 0]
    assert regular == list(range(0, regular[-1] + 1, step)) and len(starts) - len(regular) <= 1
    if overlap == 0.0:                                                               # abutting windows + the aligned tail
        assert starts[:extent // window] == list(range(0, extent - window + 1, window))
        assert len(starts) == extent // window + (1 if extent % window else 0)


def test_window_starts_of_a_short_axis():
    from boxsegliver_amd.data import lits3d
    for extent, window in ((5, 6), (6, 6), (1, 10)):
        assert lits3d.window_starts(extent, window, 0.5) == [0]
    assert lits3d.window_starts(12, 6, 0.5) == [0, 3, 6]
    assert lits3d.window_starts(40, 18, 0.5) == [0, 9, 18, 22]
    assert lits3d.window_starts(48, 22, 0.5) == [0, 11, 22, 26]


def _args(extra=""):
    from boxsegliver_amd.entry import main as entry
    return entry.get_arguments(EVAL_ARGV + extra.split())[0]


@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_eval_tables_tile_the_whole_case(ci):
    from boxsegliver_amd.data import lits3d
    store = eval3d_ref.HostStore()
    depth = ref.DEPTHS[ci]
    ch, cw = (int(v) for v in lits3d.crop_shape(SMALL[1:], (lits3d.EVAL_ZOOM, lits3d.EVAL_ZOOM)))
    assert (ch, cw) == (18, 22)
    tables = list(lits3d.eval_tables(store.meta[ci], store, SMALL, 0.5, [(0, 0, 0)], 5))
    assert all(t.dtype == np.int32 and t.shape[1] == 16 for t in tables)
    assert all(len(t) == 5 for t in tables[:-1]) and 1 <= len(tables[-1]) <= 5          # the last batch is short, not padded
    tab = np.concatenate(tables)
    zs = lits3d.window_starts(depth, 6, 0.5)
    want = [(z, y, x) for z in zs for y in (0, 9, 18, 22) for x in (0, 11, 22, 26)]
    assert len(tab) == len(want) and len(tab) % 5 != 0
    covered = np.zeros((depth, ref.H, ref.W), np.int64)
    for row, (z, y, x) in zip(tab, want):
        assert (row[0], row[1]) == (store.offset[ci], depth) and tuple(row[5:7]) == (ch, cw)
        assert tuple(row[7:10]) == (0, 0, 0) and row[11] == 0 and row[12] == 0 and not row[13:].any()
        assert np.array([row[10]], np.int32).view(np.float32)[0] == 1.0
        z1, y1, x1, bh, bw = ref.crop_box(row[2:5], row[5:7], SMALL, depth, (ref.H, ref.W))
        assert (z1, y1, x1, bh, bw) == (z, y, x, ch, cw)                              # the clamp gives back the intended start
        covered[z1:z1 + 6, y1:y1 + bh, x1:x1 + bw] += 1
    assert {w[0] for w in want} == set(zs) and min(w[1] for w in want) == 0 and max(w[1] for w in want) + ch == ref.H
    assert max(w[2] for w in want) + cw == ref.W and (max(zs) + 6 == depth or depth < 6)
    assert covered.min() >= 1                                                         # the union of the boxes is the case
    assert lits3d.table_box(tab, SMALL, depth, (ref.H, ref.W)) == (0, depth, 0, ref.H, 0, ref.W)
    assert lits3d.table_box(tab, SMALL, depth, (ref.H, ref.W)) == eval3d_ref.union_box(tab, SMALL, depth, (ref.H, ref.W))
    assert lits3d.table_box(tab[:1], SMALL, depth, (ref.H, ref.W)) == (0, min(6, depth), 0, 18, 0, 22)


def test_eval_tables_clamp_the_crop_to_the_slice():
    from boxsegliver_amd.data import lits3d
    store = eval3d_ref.HostStore()
    tab = np.concatenate(list(lits3d.eval_tables(store.meta[0], store, (6, 40, 48), 0.5, [(0, 0, 0)], 4)))
    assert len(tab) == 3 and all(tuple(r[5:7]) == (ref.H, ref.W) for r in tab)          # 45 x 54 clamped: one window in plane
    for row, z in zip(tab, (0, 3, 6)):
        assert ref.crop_box(row[2:5], row[5:7], (6, 40, 48), 12, (ref.H, ref.W)) == (z, 0, 0, ref.H, ref.W)


@pytest.mark.parametrize("flags,want", [("--eval_mirror --random_flip 7", list(range(8))),
                                        ("--eval_mirror --random_flip 1", [0, 1, 3, 5, 7]),
                                        ("--eval_mirror --random_flip 4", [0, 4, 5, 6, 7]),
                                        ("--eval_mirror --random_flip 0", [0]), ("--random_flip 7", [0])])
def test_mirror_variants_follow_the_reference(flags, want):
    from boxsegliver_amd.data import lits3d
    variants = lits3d.mirror_variants(_args(flags))
    assert variants == [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in want]
    store = eval3d_ref.HostStore()
    plain = np.concatenate(list(lits3d.eval_tables(store.meta[3], store, SMALL, 0.5, [(0, 0, 0)], 4)))
    tab = np.concatenate(list(lits3d.eval_tables(store.meta[3], store, SMALL, 0.5, variants, 4)))
    assert len(tab) == len(plain) * len(want)
    for j, row in enumerate(tab):                                                     # the same row with the flip columns set
        assert tuple(row[7:10]) == variants[j % len(want)]
        other = row.copy()
        other[7:10] = 0
        np.testing.assert_array_equal(other, plain[j // len(want)])


class _Store(eval3d_ref.HostStore):
    device = None


def test_input_fn_eval_serves_case_after_case(tmp_path):
    """Batches of the per-device batch size, the last of a case short, never two cases in one; then the end-of-case item."""
    from boxsegliver_amd.data import lits3d
    store = _Store()
    cases = [dict(m) for m in store.meta]
    args = _args("--eval_mirror --random_flip 1 --eval_skip_num 1 --eval_num 2")
    params = {"args": args, "lits_root": str(tmp_path), "device": "cpu", ("lits_store", False): (store, cases)}
    items = list(lits3d.input_fn_eval("eval", params))
    ends = [i for i, (tab, end) in enumerate(items) if tab is None]
    assert [items[i][1]["case"] for i in ends] == ["1", "2"]                          # skip one, score two
    start = 0
    for i, ci in zip(ends, (1, 2)):
        end = items[i][1]
        assert (end["base"], end["depth"]) == (store.offset[ci], ref.DEPTHS[ci]) and end["store"] is store
        tabs = [t for t, _ in items[start:i]]
        assert all(e is None for _, e in items[start:i])
        assert all(len(t) == 5 for t in tabs[:-1]) and 1 <= len(tabs[-1]) <= 5
        tab = np.concatenate(tabs)
        assert len(tab) == len(lits3d.window_starts(ref.DEPTHS[ci], 6, 0.5)) * 16 * 5
        assert (tab[:, 0] == store.offset[ci]).all() and (tab[:, 1] == ref.DEPTHS[ci]).all()
        start = i + 1
    assert start == len(items)


def test_flags_of_the_sliding_window_evaluation():
    from boxsegliver_amd.data import flagsets, lits3d
    assert "--eval_in_patches" in flagsets.PIPELINES["liver_3d"][0] and "--eval_mirror" in flagsets.PIPELINES["liver_3d"][0]
    args = _args("--eval_mirror --eval_overlap 0.5")
    assert args.eval_in_patches and args.eval_mirror and args.eval_overlap == 0.5
    assert lits3d.check_args(args) == (2, 2)
    assert _args().eval_overlap == 0.5 and not _args().eval_mirror
    assert lits3d.check_args(_args("--eval_overlap 0")) == (2, 2)
    for bad in ("1.0", "-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="eval_overlap"):
            lits3d.check_args(_args("--eval_overlap " + bad))
    with pytest.raises(ValueError, match="eval_overlap"):
        lits3d.input_fn_eval("eval", {"args": _args("--eval_overlap 1.0")})
    # the other way of the reference (one forward over the case) stays unbuilt, and so does prediction
    plain = _args()
    plain.eval_in_patches = False
    with pytest.raises(NotImplementedError, match="whole-volume 3-D evaluation"):
        lits3d.input_fn_eval("eval", {"args": plain})
    with pytest.raises(NotImplementedError):
        lits3d.input_fn_eval("infer", {"args": _args()})


def test_restatement_places_and_counts():
    """eval3d_ref.accumulate on zoom-1 rows is a plain placement: checked against slicing by hand, flips included, the
    shallow case cut at its depth, overlapping rows summed."""
    rng = np.random.default_rng(3)
    probs = rng.integers(0, 8, size=(3, 6, 16, 20, 2)).astype(np.float64)
    tab = np.stack([ref.table_row(0, 5, (2, 17, 21), (16, 20), (0, 0, 0)), ref.table_row(0, 5, (4, 39, 0), (16, 20), (1, 0, 1)),
                    ref.table_row(0, 5, (2, 19, 23), (16, 20), (0, 1, 0))])
    acc, cnt = eval3d_ref.accumulate(tab, probs, SMALL, 5, (ref.H, ref.W))
    want = np.zeros((5, ref.H, ref.W, 2))
    want[:, 9:25, 11:31] += probs[0, :5]
    want[:, 24:40, 0:20] += probs[1, ::-1, :, ::-1][:5]
    want[:, 11:27, 13:33] += probs[2, :, ::-1][:5]
    np.testing.assert_array_equal(acc, want)
    assert cnt.max() == 3 and cnt.sum() == 3 * 5 * 16 * 20 and cnt[0, 0, 47] == 0
    assert eval3d_ref.union_box(tab, SMALL, 5, (ref.H, ref.W)) == (0, 5, 9, 40, 0, 33)
    # zoomed rows: the identity at the corners of the crop (align_corners), the coverage of the crop box
    zt = np.stack([ref.table_row(0, 12, (6, 19, 23), (18, 22), (1, 1, 1))])
    zp = rng.random((1, 6, 16, 20, 1))
    acc, cnt = eval3d_ref.accumulate(zt, zp, SMALL, 12, (ref.H, ref.W))
    z1, y1, x1, ch, cw = ref.crop_box((6, 19, 23), (18, 22), SMALL, 12, (ref.H, ref.W))
    assert cnt.sum() == 6 * 18 * 22 and acc[z1, y1, x1, 0] == zp[0, 5, 15, 19, 0]
    assert acc[z1 + 5, y1 + 17, x1 + 21, 0] == zp[0, 0, 0, 0, 0]
    assert np.all(eval3d_ref.bound(acc, cnt, 1.0)[cnt == 0] == 0)
