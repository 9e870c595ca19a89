"""GPU: the 3-D interactive evaluator -- the click step `unetk_inter_click3d` (csrc/inter_eval3d.hip), the
guide of a case's windows from its click lists `unetk_click_guide3d_list`, the session loop of entry/main_eval_3d.py and the
entry point end to end.

The clicks the reference itself places are pinned by tests/golden/ref_inter_eval3d.json (made by
tests/golden/make_inter_eval3d_fixtures.py from the reference's own inter_simulation_test / update_guide / compute_dice); those
tests use the records alone.  Where the reference asks for a skeleton the click is the project's own rule, and the kernel is
held to the restatement (inter_eval3d_ref.py), which tests/test_inter_eval3d_host.py holds to the same records."""
import json
import os

import numpy as np
import pytest
import torch

import guardbuf
import inter_eval3d_ref as ref
import inter_eval3d_shapes as shapes
import lits3d_clicks_ref as cref
import lits3d_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LB_SCALE = 64
SENT = 0x7BADBAD
TAB = 20
STATE = 17


@pytest.fixture(scope="module")
def records():
    with open(os.path.join(HERE, "golden", "ref_inter_eval3d.json")) as f:
        return json.load(f)


class _GuardedInts(object):
    """An integer array inside a sentinel-filled allocation: a write outside the view is seen."""

    def __init__(self, data, dtype=torch.int32):
        data = np.ascontiguousarray(data)
        n, g = data.size, 4096
        self.flat = torch.full((n + 2 * g,), SENT, dtype=dtype, device="cuda")
        self.view = self.flat[g:g + n].view(data.shape)
        self.view.copy_(torch.from_numpy(data))
        self.snap = self.flat.clone()
        self.g, self.n = g, n

    def guard_intact(self):
        return bool(torch.equal(self.flat[:self.g], self.snap[:self.g]) and torch.equal(self.flat[self.g + self.n:], self.snap[self.g + self.n:]))


def _step(lab, pred, k=4, prev=None, pts0=None, cnt0=None, cap=255, before=2, after=1, base=None, zero_pred=False):
    """One unetk_inter_click3d call on a store that holds the case `lab` ([d, h, w] mask) after `before` and ahead of `after`
    all-object slices (so a read outside the case would be seen in the counts).  pred [d, h, w] or None (NULL; zero_pred: an
    all-zero volume instead).  Every output and a workspace of exactly the queried size sit inside guard bands; the call runs
    twice and must give identical bits.  Returns numpy arrays."""
    from boxsegliver_amd import ops
    d, h, w = lab.shape
    full = np.ones((1, h, w), np.uint8)
    lb = torch.from_numpy(np.concatenate([full] * before + [lab.astype(np.uint8)] + [full] * after) * LB_SCALE).cuda()
    base = before if base is None else base
    dp = None if pred is None else torch.from_numpy(np.ascontiguousarray(pred, dtype=np.uint8)).cuda()
    if pred is None and zero_pred:
        dp = torch.zeros((d, h, w), dtype=torch.uint8, device="cuda")
    pts0 = np.full((2, k, 3), -1, np.int32) if pts0 is None else pts0
    cnt0 = np.zeros(2, np.int32) if cnt0 is None else cnt0
    desc = ops.inter_click3d_desc(lb, base, d, k, 1, LB_SCALE, cap)
    runs = []
    for _ in range(2):
        pts, cnt = _GuardedInts(pts0), _GuardedInts(cnt0)
        table = _GuardedInts(np.full(TAB, SENT, np.int32))
        ws = guardbuf.GuardedWorkspace(ops.inter_click3d_ws(desc, "cuda").numel())
        ws.fill(0xCD)
        ops.inter_click3d(lb, base, d, dp, prev, pts.view, cnt.view, 1, LB_SCALE, cap, table.view, ws.buf[ws.off:ws.off + ws.nbytes])
        torch.cuda.synchronize()
        assert pts.guard_intact() and cnt.guard_intact() and table.guard_intact() and ws.guard_intact()
        runs.append(dict(table=table.view.cpu().numpy(), pts=pts.view.cpu().numpy(), cnt=cnt.view.cpu().numpy()))
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key], runs[1][key], err_msg="two calls differ in " + key)
    return runs[0]


def _check(out, lab, pred, msg, k=4, prev=None, pts0=None, cnt0=None, cap=255):
    """The whole table row and the click lists against the restatement."""
    pred = np.zeros_like(lab) if pred is None else pred
    have = (0, 0) if cnt0 is None else cnt0
    row, kind, click, appended = ref.table_row(pred, lab, prev, have, k, cap)
    assert out["table"].tolist() == row.tolist(), msg
    pts = np.full((2, k, 3), -1, np.int32) if pts0 is None else pts0.copy()
    cnt = np.zeros(2, np.int32) if cnt0 is None else np.array(cnt0, np.int32)
    if appended:
        pts[kind, cnt[kind]] = click
        cnt[kind] += 1
    np.testing.assert_array_equal(out["pts"], pts, err_msg=msg)
    np.testing.assert_array_equal(out["cnt"], cnt, err_msg=msg)
    return row


# ------------------------------------------------------------------------------------------------- the click step
def test_pinned_clicks_are_the_references(records):
    """Every click the reference placed itself.  Records alone: no restatement."""
    n = 0
    for r in records["singles"]:
        if r["fallback"]:
            continue
        lab, pred = shapes.build(r["shape"], r["ref"]), shapes.build(r["shape"], r["pred"])
        out = _step(lab, pred if r["pred"] else None)
        row, msg = out["table"], "{} {}".format(r["name"], r["shape"])
        assert row[STATE] == 1 and row[15] == 0 and row[13] == 0 and row[16] == 1, msg
        assert row[9:13].tolist() == r["click"] + [r["kind"]], msg
        assert out["cnt"].tolist() == [1 - r["kind"], r["kind"]] and out["pts"][r["kind"], 0].tolist() == r["click"], msg
        n += 1
    assert n >= 18


def test_every_record_equals_the_restatement(records):
    """The whole table row, fallback clicks included (the project's rule), at the three fixture shapes."""
    seen = set()
    for r in records["singles"]:
        lab, pred = shapes.build(r["shape"], r["ref"]), shapes.build(r["shape"], r["pred"])
        row = _check(_step(lab, pred), lab, pred, "{} {}".format(r["name"], r["shape"]))
        assert bool(row[13]) == r["fallback"]
        seen.add((tuple(r["shape"]), bool(row[13]), int(row[12])))
    for shape in ((6, 20, 24), (12, 40, 48), (20, 64, 70)):
        assert {(shape, True, 0), (shape, True, 1), (shape, False, 0), (shape, False, 1)} <= seen


def _edge_cases():
    """(name, ref, pred or None): depth 1, the extent limits, a union-find that needs many rounds, an empty error mask."""
    flat = shapes.build((1, 20, 24), [["+", "box", 0, 1, 2, 18, 3, 21], ["-", "box", 0, 1, 8, 12, 8, 16]])    # the mean lies in the hole
    wide = np.zeros((3, 1024, 9), np.uint8)
    wide[:, 1:1023, 1:8] = 1
    wide[1, 20:1000, 3:6] = 0
    long_ = np.zeros((3, 9, 1024), np.uint8)
    long_[:, 2:8, 3:1021] = 1
    long_[:, 4:6, 100:900] = 0
    sp = shapes.spiral(4, 21, 23)
    blob = shapes.build((6, 20, 24), shapes.two_ellipsoids((6, 20, 24)))
    return [("depth 1", flat, None), ("depth 1 bg", np.zeros_like(flat), flat), ("3x1024x9", wide, None), ("3x9x1024", long_, None),
            ("3x9x1024 bg", np.zeros_like(long_), long_), ("spiral", sp, None), ("spiral bg", np.zeros_like(sp), sp),
            ("empty", blob, blob), ("empty zero", np.zeros_like(blob), None)]


@pytest.mark.parametrize("name", [c[0] for c in _edge_cases()])
def test_edge_shapes_equal_the_restatement(name):
    _, r, p = [c for c in _edge_cases() if c[0] == name][0]
    want = ref.click(np.zeros_like(r) if p is None else p, r)
    if name.startswith("spiral"):
        assert want["n_comp"] == 1 and want["area"] == int(shapes.spiral(4, 21, 23).sum()) and want["fallback"]
    if name.startswith("empty"):
        assert want["empty"]
    if name.startswith("3x") or name.startswith("depth 1"):
        assert want["fallback"]
    out = _step(r, p)
    row = _check(out, r, p, name)
    assert row[16] == (0 if want["empty"] else 1)
    if want["empty"]:
        assert out["cnt"].tolist() == [0, 0] and (out["pts"] == -1).all()


def test_the_cap_decides_ties_by_the_candidate_then_the_index():
    """12 x 40 x 48 with dist_cap = 3: a block 5 deep and more around a hole at its mean; every voxel 3 or more inside ties
    at the cap, so the arg-max is decided by the squared distance to the candidate, then by the index."""
    lab = shapes.build((12, 40, 48), [["+", "box", 1, 11, 4, 36, 4, 44], ["-", "box", 5, 7, 19, 21, 23, 25]])
    free = ref.click(np.zeros_like(lab), lab)
    capped = ref.click(np.zeros_like(lab), lab, cap=3)
    assert free["fallback"] and capped["fallback"] and free["cand"] == (6, 20, 24) and free["click"] != capped["click"]
    assert int(ref.city_block(lab.astype(bool)).max()) > 3
    _check(_step(lab, None, cap=3), lab, None, "cap 3", cap=3)
    _check(_step(lab, None), lab, None, "cap 255")
    _check(_step(np.zeros_like(lab), lab, cap=1), np.zeros_like(lab), lab, "cap 1, background", cap=1)


def test_full_lists_repeats_and_a_case_outside_the_store(records):
    rec = [r for r in records["singles"] if r["name"] == "object" and r["shape"] == [6, 20, 24]][0]
    lab = shapes.build(rec["shape"], rec["ref"])
    click = tuple(rec["click"])
    k = 2
    pts0 = np.full((2, k, 3), -1, np.int32)
    pts0[0] = [[1, 1, 1], [2, 2, 2]]
    cnt0 = np.array([k, 0], np.int32)
    out = _step(lab, None, k=k, prev=click, pts0=pts0, cnt0=cnt0)                   # the list is full; the click repeats
    row = _check(out, lab, None, "full", k=k, prev=click, pts0=pts0, cnt0=cnt0)
    assert row[14] == 1 and row[16] == 0 and row[9:12].tolist() == list(click)
    near = (click[0], click[1], click[2] + 1)
    cnt1 = np.array([1, 0], np.int32)
    out = _step(lab, None, k=k, prev=near, pts0=pts0, cnt0=cnt1)                    # next to it: no repeat; appended at slot 1
    row = _check(out, lab, None, "near", k=k, prev=near, pts0=pts0, cnt0=cnt1)
    assert row[14] == 0 and row[16] == 1 and out["pts"][0, 1].tolist() == list(click)
    out = _step(lab, None, k=k, cnt0=np.array([-5, 99], np.int32))                  # counts out of range are clamped
    assert out["table"][16] == 1 and out["cnt"].tolist() == [1, 99] and out["pts"][0, 0].tolist() == list(click)
    for base in (-1, 4, 100):                                                        # the store holds 2 + 6 + 1 slices
        out = _step(lab, None, k=k, pts0=pts0, cnt0=cnt1, base=base)
        want = np.zeros(TAB, np.int32)
        want[5:13], want[STATE] = -1, 2
        assert out["table"].tolist() == want.tolist(), base
        np.testing.assert_array_equal(out["pts"], pts0)
        assert out["cnt"].tolist() == cnt1.tolist()
    out = _step(lab, None, before=0, after=0)                                        # the case is the whole store
    _check(out, lab, None, "whole store")


def test_null_prediction_is_an_all_zero_prediction(records):
    for r in records["singles"][:3]:
        lab = shapes.build(r["shape"], r["ref"])
        a, b = _step(lab, None), _step(lab, None, zero_pred=True)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key])


def test_a_short_workspace_is_refused():
    from boxsegliver_amd import _abi, ops
    lb = torch.zeros((6, 20, 24), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((2, 4, 3), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    nbytes = ops.inter_click3d_ws(ops.inter_click3d_desc(lb, 0, 6, 4), "cuda").numel()
    assert nbytes == 512 + 3072 + 2 * 11520                          # header, info; 2880 err bytes (rounded to 256), labels, sizes
    with pytest.raises(_abi.UnetkError):
        ops.inter_click3d(lb, 0, 6, None, None, pts, cnt, ws=torch.empty(nbytes - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_abi.UnetkError):
        ops.inter_click3d_ws(ops.inter_click3d_desc(lb, 0, 6, 65), "cuda")


# ------------------------------------------------------------------------------------------------- the guide from lists
SRC = (lits3d_ref.H, lits3d_ref.W)
FLIPS = [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in range(8)]


def _rows(depth, shape, flips_list):
    """One row per flip set: windows at different places of a case of `depth` slices at store slice 3 (zoomed crops)."""
    rows, boxes = [], []
    for j, flips in enumerate(flips_list):
        centre = ((2 + 3 * j) % max(depth, 1), (7 + 11 * j) % SRC[0], (5 + 13 * j) % SRC[1])
        crop = (18 + (j % 3) * 7, 22 + (j % 2) * 9)
        rows.append(lits3d_ref.table_row(3, depth, centre, crop, flips))
        boxes.append(lits3d_ref.crop_box(centre, crop, shape, depth, SRC))
    return np.stack(rows), boxes


def _case_clicks(n, depth, salt):
    """n clicks spread over the case (so most lie outside any one window's box, in z, y and x), from integers: int32 [n, 3]."""
    return np.array([((5 * i + salt) % depth, (7 * i * i + 3 * i + salt) % SRC[0], (11 * i + 5 * salt + i * i) % SRC[1]) for i in range(n)],
                    np.int32).reshape(n, 3)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0)])
def test_guide_list_equals_click_guide3d_up_to_four_clicks(channels, stddev):
    """Bit for bit against unetk_click_guide3d fed the same clicks relative to each row's box, under all eight flips."""
    from boxsegliver_amd import ops
    shape, depth = (6, 16, 20), 12
    tab, boxes = _rows(depth, shape, FLIPS)
    dtab = torch.from_numpy(tab).cuda()
    for counts in ((0, 0), (1, 0), (0, 3), (4, 4), (2, 1)):
        case_pts = np.full((2, 4, 3), -1, np.int32)
        for kind in range(2):
            case_pts[kind, :counts[kind]] = _case_clicks(counts[kind], depth, 3 + kind)
        rel = np.stack([case_pts - np.array(b[:3], np.int32) for b in boxes])           # [N, 2, 4, 3]
        cnt = np.array(counts, np.int32)
        want = ops.click_guide3d(dtab, torch.from_numpy(rel).cuda(), torch.from_numpy(np.tile(cnt, (len(boxes), 1))).cuda(), shape, SRC,
                                 channels, stddev)
        for k in (4, 7, 64):
            pk = np.full((2, k, 3), 12345, np.int32)                                    # the slots past the counts are not read
            pk[:, :4] = case_pts
            got = ops.click_guide3d_list(dtab, torch.from_numpy(pk).cuda(), torch.from_numpy(cnt).cuda(), shape, SRC, channels, stddev)
            assert got.shape == (8,) + shape + (channels,)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (counts, k)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0)])
@pytest.mark.parametrize("depth", [12, 4])
def test_guide_list_with_many_clicks_matches_float64(channels, stddev, depth):
    """5, 20 and 64 clicks per kind, and a kind without clicks, under the bounds of the 2-D list guide: Gaussian 2e-6,
    Euclidean 8 * 2^-24 * max(1, largest distance).  depth 4 < D = 6: a shallow case, whose box starts at slice 0."""
    from boxsegliver_amd import ops
    shape, k = (6, 16, 20), 64
    flips_list = [FLIPS[0], FLIPS[7], FLIPS[2], FLIPS[5]]
    tab, boxes = _rows(depth, shape, flips_list)
    dtab = torch.from_numpy(tab).cuda()
    norm = cref.euclid_norm(shape[1])
    for counts in ((5, 20), (64, 0), (0, 64), (20, 5)):
        pts = np.full((2, k, 3), -1, np.int32)
        for kind in range(2):
            pts[kind, :counts[kind]] = _case_clicks(counts[kind], depth, 5 + kind)
        got = ops.click_guide3d_list(dtab, torch.from_numpy(pts).cuda(), torch.from_numpy(np.array(counts, np.int32)).cuda(), shape, SRC,
                                     channels, stddev).cpu().numpy()
        outside = False
        for j, (box, flips) in enumerate(zip(boxes, flips_list)):
            rel = pts - np.array(box[:3], np.int32)
            live = np.concatenate([rel[kind, :counts[kind]] for kind in range(2)])
            outside |= bool((live < 0).any(axis=0).all() and (live[:, 0] >= shape[0]).any())
            want, far = cref.sp_guide((shape[0],) + box[3:], shape[1:], rel, counts, flips, stddev, channels, norm)
            bound = 2e-6 if stddev is not None else 8 * 2.0 ** -24 * max(1.0, far)
            err = np.abs(got[j].astype(np.float64) - want).max()
            assert err <= bound, (counts, j, err, bound)
            if channels == 2:
                for kind in range(2):
                    if counts[kind] == 0:
                        assert (got[j, ..., kind] == 0).all()
        assert outside or depth < shape[0]                                              # outside a box in z, y and x


def test_guide_list_guard_bands():
    from boxsegliver_amd import ops
    shape, depth, k = (6, 16, 20), 12, 20
    tab, _ = _rows(depth, shape, FLIPS[:3])
    pts = _GuardedInts(np.concatenate([_case_clicks(k, depth, 1), _case_clicks(k, depth, 2)]).reshape(2, k, 3))
    cnt = _GuardedInts(np.array([k + 50, -3], np.int32))                                # clamped into [0, K]
    got = ops.click_guide3d_list(torch.from_numpy(tab).cuda(), pts.view, cnt.view, shape, SRC, 2, (1.0, 3.0, 3.0))
    full = ops.click_guide3d_list(torch.from_numpy(tab).cuda(), pts.view, torch.tensor([k, 0], dtype=torch.int32, device="cuda"), shape,
                                  SRC, 2, (1.0, 3.0, 3.0))
    torch.cuda.synchronize()
    assert torch.equal(got, full) and (got[..., 1] == 0).all() and pts.guard_intact() and cnt.guard_intact()
    assert torch.equal(pts.flat, pts.snap) and torch.equal(cnt.flat, cnt.snap)          # inputs only


# ------------------------------------------------------------------------------------------------- the session loop
def test_recorded_sessions_through_the_session_loop(records):
    """Click for click, counter for counter and stop reason for stop reason: the sessions the reference ran
    (make_inter_eval3d_fixtures.run_session), the repeat session among them.  A recorded session was followed up to its first
    fallback round; there the loop must report a fallback click."""
    from boxsegliver_amd.entry import main_eval_3d
    seen_stops = set()
    for s in list(records["sessions"]) + [records["repeat"]]:
        shape = tuple(s["shape"])
        lab = shapes.build(shape, s["ref"])
        lb = torch.from_numpy(np.concatenate([np.ones((1,) + shape[1:], np.uint8), lab]) * LB_SCALE).cuda()   # the case starts at slice 1

        def toy(fg, bg, s=s, shape=shape):
            if "pred" in s:
                return shapes.build(shape, s["pred"])
            return shapes.ball_prediction(shape, fg, bg, s["r_fg"], s["r_bg"])

        def predict(pts, cnt, toy=toy):
            p, c = pts.cpu().numpy(), cnt.cpu().numpy()
            return torch.from_numpy(toy(p[0, :c[0]], p[1, :c[1]])).cuda()
        trace = []
        inters, last = main_eval_3d.run_session(lb, 1, shape[0], predict, s["max_iter"], s["inter_thresh"], 1, trace, "toy")
        n = [sum(1 for r in trace if r[1] is not None and r[2] == kind) for kind in range(2)]
        assert inters == n
        for i, want in enumerate(s["rounds"]):
            assert list(trace[i][1]) == want["click"] and trace[i][2] == want["kind"] and not trace[i][3], (shape, i)
            assert list(trace[i + 1][4]) == want["counts"], (shape, i)                   # read with the next click
        at = trace[len(s["rounds"])]
        seen_stops.add(s["stop"])
        if s["stop"] == "fallback":
            assert at[3] and at[1] is not None, shape
        else:
            assert at[5] == s["stop"] and len(trace) == len(s["rounds"]) + 1 and n == s["num_iter"], (shape, at)
        assert trace[-1][5] is not None and all(r[5] is None for r in trace[:-1])
        # the whole session equals the restatement's, fallback rounds included
        rounds, stop, num_iter = ref.session(lab, toy, s["inter_thresh"], s["max_iter"])
        assert stop == trace[-1][5] and num_iter == n
        assert [(r[0], r[1], r[2]) for r in rounds] == [(t[1], t[2], t[3]) for t in trace if t[1] is not None][:len(rounds)]
    assert seen_stops == {"fallback", "repeat"}


# ------------------------------------------------------------------------------------------------- end to end
def _eval_argv(root, classes, extra):
    argv = ("--mode eval --tag inter3d --model UNet3D --classes {} --test_fold 1 --im_depth 4 --im_height 32 --im_width 32 "
            "--im_channel 1 --batch_size 8 --normalizer instance_norm --metrics_eval Dice VOE --inter_thresh 0.9 "
            "--eval_overlap 0.0").format(classes).split()
    return argv + extra + ["--lits_root", str(root), "--model_dir", str(root / "run")]


@pytest.mark.parametrize("classes,extra,scored", [
    ("Liver", "--use_spatial --local_enhance --stddev 1 3 3 --eval_mirror --random_flip 4 --max_iter 2", [2, 3]),
    ("Liver Tumor", "--use_spatial --guide_channel 1 --max_iter 3", [2, 3]),
    ("Tumor", "--use_spatial --local_enhance --guide_channel 1 --eval_mirror --random_flip 1 --max_iter 0 --infer_set train", [0]),
    ("Tumor", "--use_spatial --max_iter 2 --eval_window_weight gaussian --infer_set train", [0]),
])
def test_main_eval_3d_end_to_end_at_random_weights(tmp_path, classes, extra, scored):
    from boxsegliver_amd import loss_metrics
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main_eval_3d
    cases = lits3d_ref.write_dataset(tmp_path)
    args = main_eval_3d.get_arguments(_eval_argv(tmp_path, classes, extra.split()))
    rf = int(args.random_flip) if args.eval_mirror else 0
    assert len(lits3d.mirror_variants(args)) == {0: 1, 4: 5, 1: 5}[rf]                # run_TTA: every m in 1..7 with (random_flip & m) > 0
    trace, volumes = [], {}
    results = main_eval_3d.run(args, trace=trace, trace_preds=True, restore=False, volumes=volumes)
    obj = 2 if "Tumor" in classes else 1
    n_cls = len(classes.split())
    assert sorted(volumes) == scored                                  # --infer_set train: case 1 holds no tumour and is skipped
    cls = classes.split()[-1]
    per_metric = {"Dice": [], "VOE": []}
    tp = fp = fn = 0
    clicks = [0, 0]
    for pid in scored:
        label = (cases[pid][1] >= obj).astype(np.uint8)
        raw = volumes[pid].cpu().numpy()
        assert raw.shape == label.shape and raw.dtype == np.uint8 and raw.max() <= n_cls
        v = (raw >= n_cls).astype(np.uint8)
        for key, value in loss_metrics.metric_3d(v, label, required=["Dice", "VOE"]).items():
            per_metric[key].append(value)
        tp, fp, fn = tp + int((v & label).sum()), fp + int((v & ~label & 1).sum()), fn + int((~v & label & 1).sum())
        rounds = [r for r in trace if r[0] == pid]
        assert rounds[-1][5] in ("repeat", "dice", "max_iter", "empty") and all(r[5] is None for r in rounds[:-1])
        assert rounds[0][6] is None                                                       # round 0: all zeros
        prev, n = None, [0, 0]
        for r in rounds:
            pred = np.zeros_like(label) if r[6] is None else r[6]
            row, kind, click, _ = ref.table_row(pred, label, prev)
            assert r[4] == tuple(row[:3]), pid
            if r[1] is not None:
                assert (r[1], r[2], r[3]) == (click, kind, bool(row[13])), pid
                assert (r[5] == "repeat") == bool(row[14])
                n[kind] += 1
                prev = click
            if r[5] == "dice":
                assert ref.dice(*r[4]) > 0.9
        assert sum(n) <= max(int(args.max_iter), 1)
        if int(args.max_iter) == 0:                                                       # one click, one forward, then --max_iter stops it
            assert [r[5] for r in rounds] == [None, "max_iter"] and n == [1, 0]
        if len(rounds) > 1:
            np.testing.assert_array_equal(v, rounds[-1][6])                               # the last forward's
        clicks = [clicks[0] + n[0], clicks[1] + n[1]]
    for key, values in per_metric.items():
        assert results["{}/{}".format(cls, key)] == pytest.approx(float(np.mean(values)), rel=1e-12, abs=1e-12)
    assert results["G_Dice"] == pytest.approx(2 * tp / (2 * tp + fn + fp) if tp + fn + fp else 0.0, rel=1e-12)
    assert (results["inters_fg"], results["inters_bg"]) == (clicks[0] / len(scored), clicks[1] / len(scored))
    text = open(str(tmp_path / "run" / "logs" / "eval_inter3d")).read()
    assert "Evaluate-{} ".format(scored[0]) in text and "(Num inters: [" in text and "(Average inters: " in text
    assert "---Infer {} cases".format(len(scored)) in text


def test_without_use_spatial_the_volumes_are_run_3ds(tmp_path, monkeypatch):
    """One pass and no clicks: after two training steps, `liver_3d --mode eval --eval_in_patches` and main_eval_3d score the same
    checkpoint with the same arguments; the class volumes that run_3d hands to its post-processing and the ones main_eval_3d
    returns are equal bit for bit -- the window loop is shared."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval_3d
    lits3d_ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    common = ("--tag cli3d --model UNet3D --classes Liver --test_fold 1 --im_depth 4 --im_height 32 --im_width 32 --im_channel 1 "
              "--random_flip 7 --normalizer instance_norm").split() + ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    train = ("liver_3d --mode train --tumor_percent 0.5 --batch_size 2 --num_of_steps 2 --batches_per_epoch 2 --evaluator Volume "
             "--loss_weight_type numerical --loss_numeric_w 1 1 --learning_rate 0.001 --log_step 1").split()
    assert entry.main(train + common) == 0
    ev = "--mode eval --batch_size 8 --eval_in_patches --eval_mirror --eval_final --metrics_eval Dice".split() + common
    volumes_3d = []
    real_predict = ops.head_predict

    def recording_predict(probs, ncls, want_preds=True):
        out = real_predict(probs, ncls, want_preds)
        if not want_preds:
            volumes_3d.append(out[0].clone())
        return out
    monkeypatch.setattr(ops, "head_predict", recording_predict)
    args, sub, pipe = entry.get_arguments(["liver_3d", "--evaluator", "Volume"] + ev)
    entry.run(args, sub, pipe)
    monkeypatch.undo()
    assert len(volumes_3d) == 2
    volumes, trace = {}, []
    results = main_eval_3d.run(main_eval_3d.get_arguments(ev), trace=trace, volumes=volumes)
    assert sorted(volumes) == [2, 3] and not trace and (results["inters_fg"], results["inters_bg"]) == (0.0, 0.0)
    for pid, got in zip((2, 3), volumes_3d):
        assert torch.equal(volumes[pid].flatten(), got.flatten()) and volumes[pid].shape == (lits3d_ref.DEPTHS[pid],) + SRC
    assert 0.0 <= results["Liver/Dice"] <= 1.0 and 0.0 <= results["G_Dice"] <= 1.0
    with pytest.raises(FileNotFoundError, match="Missing checkpoint"):
        main_eval_3d.run(main_eval_3d.get_arguments([a if a != str(run) else str(tmp_path / "none") for a in ev]))
