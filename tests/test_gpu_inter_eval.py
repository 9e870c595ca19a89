"""GPU: the interactive evaluator -- the click step `unetk_inter_click` (csrc/inter_eval.hip), the guide
from click lists `unetk_click_guide_list`, the session loop of entry/main_eval.py and the entry point end to end.

The clicks the reference itself places are pinned by tests/golden/ref_inter_eval.json (made by
tests/golden/make_inter_eval_fixtures.py from the reference's own inter_simulation_test / update_guide / compute_dice); those
tests use the records alone.  Where the reference asks for a skeleton the click is the project's own rule, and the kernel is
held to the restatement (inter_eval_ref.py), which tests/test_inter_eval_host.py holds to the same records."""
import json
import os

import numpy as np
import pytest
import torch

import guardbuf
import inter_eval_ref as ref
import inter_eval_shapes as shapes
import lits_inter_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LB_SCALE = 64
SENT = 0x7BADBAD
COLS = dict(n_pred=0, n_ref=1, n_inter=2, n_comp=3, area=4, root=5, cy=6, cx=7, y=8, x=9, kind=10, fallback=11, repeat=12,
            empty=13, appended=14, state=15)


@pytest.fixture(scope="module")
def records():
    with open(os.path.join(HERE, "golden", "ref_inter_eval.json")) as f:
        return json.load(f)


class _GuardedInts(object):
    """An integer array inside a sentinel-filled allocation: a write outside the view is seen."""

    def __init__(self, data, dtype):
        data = np.ascontiguousarray(data)
        n, g = data.size, 4096
        self.flat = torch.full((n + 2 * g,), SENT if dtype == torch.int32 else 0xAB, dtype=dtype, device="cuda")
        self.view = self.flat[g:g + n].view(data.shape)
        self.view.copy_(torch.from_numpy(data))
        self.snap = self.flat.clone()
        self.g, self.n = g, n

    def guard_intact(self):
        return bool(torch.equal(self.flat[:self.g], self.snap[:self.g]) and torch.equal(self.flat[self.g + self.n:], self.snap[self.g + self.n:]))


def _step(refs, preds, k=4, active=None, prev=None, pts0=None, cnt0=None, slices=None, vol_base=0):
    """One unetk_inter_click call on a store made of `refs` ([n][h, w] masks): session j works on store slice slices[j] (j by
    default) with prediction preds[j] (all [H, W] alike, or None for all).  Every output and a workspace of exactly the queried
    size sit inside guard bands; the call runs twice and must give identical bits.  Returns numpy arrays."""
    from boxsegliver_amd import ops
    n_store = len(refs)
    h, w = refs[0].shape
    lb = torch.from_numpy(np.stack(refs).astype(np.uint8) * LB_SCALE).cuda()
    slices = list(range(n_store)) if slices is None else list(slices)
    n = len(slices)
    rows = np.zeros((n, 4), np.int32)
    rows[:, 0] = slices
    rows[:, 1] = 1 if active is None else active
    rows[:, 2:] = -1 if prev is None else prev
    pred = None if preds is None else torch.from_numpy(np.stack(preds).astype(np.uint8)).cuda()
    pred_hw = (h, w) if preds is None else preds[0].shape
    pts0 = np.full((n, 2, k, 2), -1, np.int32) if pts0 is None else pts0
    cnt0 = np.zeros((n, 2), np.int32) if cnt0 is None else cnt0
    desc = ops.inter_click_desc(lb, n, pred_hw, k, 1, LB_SCALE, vol_base, n_store - vol_base)
    runs = []
    for _ in range(2):
        pts, cnt = _GuardedInts(pts0, torch.int32), _GuardedInts(cnt0, torch.int32)
        table = _GuardedInts(np.full((n, 16), SENT, np.int32), torch.int32)
        vol = _GuardedInts(np.full((n_store - vol_base, h, w), 0xAB, np.uint8), torch.uint8)
        ws = guardbuf.GuardedWorkspace(ops.inter_click_ws(desc, "cuda").numel())
        ws.fill(0xCD)
        ops.inter_click(lb, torch.from_numpy(rows).cuda(), pred, pts.view, cnt.view, 1, LB_SCALE, vol.view, vol_base, pred_hw,
                        table.view, ws.buf[ws.off:ws.off + ws.nbytes])
        torch.cuda.synchronize()
        assert pts.guard_intact() and cnt.guard_intact() and table.guard_intact() and vol.guard_intact() and ws.guard_intact()
        runs.append(dict(table=table.view.cpu().numpy(), pts=pts.view.cpu().numpy(), cnt=cnt.view.cpu().numpy(),
                         vol=vol.view.cpu().numpy()))
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key], runs[1][key], err_msg="two calls differ in " + key)
    return runs[0]


def _check_row(row, c, msg):
    """A table row against inter_eval_ref.click's dict."""
    want = [c["counts"][0], c["counts"][1], c["counts"][2], c["n_comp"], c["area"], c["root"], c["cand"][0], c["cand"][1],
            c["click"][0], c["click"][1], c["kind"], int(c["fallback"]), int(c["empty"])]
    assert row[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13]].tolist() == want, msg


def _by_shape(singles):
    out = {}
    for r in singles:
        out.setdefault(tuple(r["shape"]), []).append(r)
    return out


# ------------------------------------------------------------------------------------------------- the click step
def test_pinned_clicks_are_the_references(records):
    """Every click the reference placed itself, one launch per shape (40 x 48: one trip of every loop; 100 x 104: a full and a
    ragged trip; 140 x 333: a row wider than a block).  Records alone: no restatement."""
    for shape, recs in _by_shape(records["singles"]).items():
        refs = [shapes.build(shape, r["ref"]) for r in recs]
        preds = [shapes.build(shape, r["pred"]) for r in recs]
        out = _step(refs, preds)
        for j, r in enumerate(recs):
            row = out["table"][j]
            msg = "{} {}".format(r["name"], shape)
            assert row[COLS["state"]] == 1 and row[COLS["empty"]] == 0, msg
            assert bool(row[COLS["fallback"]]) == r["fallback"], msg
            if not r["fallback"]:
                assert row[[8, 9, 10]].tolist() == r["click"] + [r["kind"]], msg
            np.testing.assert_array_equal(out["vol"][j], preds[j], err_msg=msg)
            kind = row[COLS["kind"]]
            assert out["cnt"][j].tolist() == [1 - kind, kind] and out["pts"][j, kind, 0].tolist() == row[[8, 9]].tolist(), msg


def test_every_record_equals_the_restatement(records):
    """The whole table row, fallback clicks included (the project's rule), with the prediction given at HALF resolution: the
    kernel's nearest resize against shapes.resize_nearest."""
    for shape, recs in _by_shape(records["singles"]).items():
        refs = [shapes.build(shape, r["ref"]) for r in recs]
        half = (shape[0] // 2, (shape[1] + 1) // 2)
        small = [shapes.build(half, [[i[0], i[1]] + [v // 2 for v in i[2:]] for i in r["pred"]]) for r in recs]
        full = [shapes.build(shape, r["pred"]) for r in recs]
        for preds, at_src in ((full, full), (small, [shapes.resize_nearest(p, shape) for p in small])):
            out = _step(refs, preds)
            for j, r in enumerate(recs):
                _check_row(out["table"][j], ref.click(at_src[j], refs[j]), "{} {}".format(r["name"], shape))
                np.testing.assert_array_equal(out["vol"][j], at_src[j])


def _edge_cases():
    """(name, ref, pred or None): the extent limits, a union-find that needs many rounds, an empty error mask."""
    wide = np.zeros((12, 1024), np.uint8)
    wide[2:10, 3:1021] = 1
    wide[4:8, 100:900] = 0                                       # a frame: the mean lies in the hole
    tall = np.zeros((1024, 9), np.uint8)
    tall[1:1023, 1:8] = 1
    tall[20:1000, 3:6] = 0
    sp = shapes.spiral(61, 67)
    blob = shapes.build((61, 67), [["+", "ellipse", 30, 30, 11, 17]])
    return [("12x1024", wide, None), ("1024x9", tall, None), ("1024x9 bg", np.zeros_like(tall), tall),
            ("spiral", sp, None), ("spiral bg", np.zeros_like(sp), sp), ("empty", blob, blob), ("empty zero", np.zeros_like(sp), None)]


@pytest.mark.parametrize("name", [c[0] for c in _edge_cases()])
def test_edge_shapes_equal_the_restatement(name):
    _, r, p = [c for c in _edge_cases() if c[0] == name][0]
    p = np.zeros_like(r) if p is None else p
    want = ref.click(p, r)
    if name.startswith("spiral"):
        assert want["n_comp"] == 1 and want["area"] == int(shapes.spiral(61, 67).sum())
    if name.startswith("empty"):
        assert want["empty"]
    out = _step([r], [p])                                        # N = 1
    _check_row(out["table"][0], want, name)
    assert out["table"][0][COLS["appended"]] == (0 if want["empty"] else 1)
    if want["empty"]:
        assert out["cnt"][0].tolist() == [0, 0] and (out["pts"][0] == -1).all()


def test_capped_distance_on_a_megapixel_component():
    """1024 x 1024, all error but a 3 x 3 hole at the mean: 2^20 - 9 pixels in one component, and the distance reaches the
    cap of 255, so the arg-max is decided by the distance to the mean and the index.  One launch (the helper's second call is
    the identical-bits check)."""
    r = np.ones((1024, 1024), np.uint8)
    r[510:513, 510:513] = 0
    want = ref.click(np.zeros_like(r), r)
    assert want["fallback"] and want["area"] == (1 << 20) - 9 and want["cand"] == (512, 512)
    out = _step([r], None)
    _check_row(out["table"][0], want, "1024 x 1024")


def test_batch_with_an_inactive_row_full_lists_and_repeats(records):
    """N = 5 on a store of 7 slices with a volume that starts at slice 1: an inactive row in the middle stays untouched, a
    full list is not appended to, the repeat flag compares with the row's previous click, a slice outside the volume is state
    2; K = 3."""
    shape = (40, 48)
    recs = [r for r in records["singles"] if tuple(r["shape"]) == shape][:7]
    refs = [shapes.build(shape, r["ref"]) for r in recs]
    preds_all = [shapes.build(shape, r["pred"]) for r in recs]
    slices = [3, 1, 5, 0, 6]                                      # slice 0 lies before the volume
    want = [ref.click(preds_all[s], refs[s]) for s in slices]
    k = 3
    pts0 = np.full((5, 2, k, 2), -1, np.int32)
    cnt0 = np.zeros((5, 2), np.int32)
    pts0[1, want[1]["kind"]] = [[1, 1], [2, 2], [3, 3]]          # row 1: its kind's list is full
    cnt0[1, want[1]["kind"]] = k
    pts0[4, want[4]["kind"], 0] = want[4]["click"]                # row 4: the click repeats
    cnt0[4, want[4]["kind"]] = 1
    prev = np.full((5, 2), -1, np.int32)
    prev[4] = want[4]["click"]
    prev[0] = [want[0]["click"][0], want[0]["click"][1] + 1]     # row 0: next to it, no repeat
    out = _step(refs, [preds_all[s] for s in slices], k=k, active=[1, 1, 0, 1, 1], prev=prev, pts0=pts0, cnt0=cnt0, slices=slices,
                vol_base=1)
    t = out["table"]
    assert t[:, COLS["state"]].tolist() == [1, 1, 0, 2, 1]
    for j in (0, 1, 4):
        _check_row(t[j], want[j], "row {}".format(j))
        np.testing.assert_array_equal(out["vol"][slices[j] - 1], preds_all[slices[j]])
    for j in (2, 3):                                              # nothing but the table row
        assert t[j, :15].tolist() == [0] * 8 + [-1, -1, -1, 0, 0, 0, 0]
        np.testing.assert_array_equal(out["pts"][j], pts0[j])
        assert out["cnt"][j].tolist() == [0, 0]
    for z in (1, 3):                                              # volume slices of no session (store slices 2 and 4)
        assert (out["vol"][z] == 0xAB).all()
    assert t[[0, 1, 4], COLS["repeat"]].tolist() == [0, 0, 1] and t[[0, 1, 4], COLS["appended"]].tolist() == [1, 0, 1]
    np.testing.assert_array_equal(out["pts"][1], pts0[1])
    assert out["cnt"][1].tolist() == cnt0[1].tolist()
    kind = want[4]["kind"]
    assert out["cnt"][4, kind] == 2 and out["pts"][4, kind, 1].tolist() == list(want[4]["click"])
    kind = want[0]["kind"]
    assert out["cnt"][0, kind] == 1 and out["pts"][0, kind, 0].tolist() == list(want[0]["click"])


def test_bad_arguments_and_the_workspace_query():
    import ctypes

    from boxsegliver_amd import _abi, ops
    lb = torch.zeros((2, 40, 48), dtype=torch.uint8, device="cuda")
    lib = _abi.lib()
    for kw in (dict(k=65), dict(k=0), dict(pred_hw=(4096, 1024))):
        args = dict(n=2, pred_hw=(20, 24), k=4)
        args.update(kw)
        desc = ops.inter_click_desc(lb, args["n"], args["pred_hw"], args["k"])
        assert lib.unetk_inter_click_ws_bytes(ctypes.byref(desc)) == 0
    big = torch.zeros((1, 1025, 8), dtype=torch.uint8, device="cuda")
    assert lib.unetk_inter_click_ws_bytes(ctypes.byref(ops.inter_click_desc(big, 1, (8, 8), 4))) == 0
    desc = ops.inter_click_desc(lb, 2, (20, 24), 4)
    nbytes = lib.unetk_inter_click_ws_bytes(ctypes.byref(desc))
    assert nbytes > 0
    rows = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    pts = torch.zeros((2, 2, 4, 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(_abi.UnetkError):                          # a workspace one byte short
        ops.inter_click(lb, rows, None, pts, cnt, pred_hw=(20, 24), ws=torch.empty(nbytes - 1, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------- the guide from lists
def _whole_slice_tab(n, src_hw):
    rows = [lits_inter_ref.table_row(0, 1, (0, src_hw[0] // 2, src_hw[1] // 2), src_hw) for _ in range(n)]
    return torch.from_numpy(np.stack(rows)).cuda()


def _spread_clicks(n, src_hw, salt):
    """n clicks spread over the slice, from integers: int32 [n, 2]."""
    h, w = src_hw
    return np.array([((7 * i * i + 3 * i + salt) % h, (11 * i + 5 * salt + i * i) % w) for i in range(n)], np.int32).reshape(n, 2)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("stddev", [None, 5.0])
def test_guide_list_equals_click_guide_up_to_four_clicks(channels, stddev):
    from boxsegliver_amd import ops
    src, out_hw = (40, 48), (32, 24)
    counts = [(0, 0), (1, 0), (0, 3), (4, 4), (2, 1)]
    tab = _whole_slice_tab(len(counts), src)
    p4 = np.full((len(counts), 2, 4, 2), -1, np.int32)
    for j, c in enumerate(counts):
        for kind in range(2):
            p4[j, kind, :c[kind]] = _spread_clicks(c[kind], src, 3 * j + kind)
    cnt = torch.from_numpy(np.array(counts, np.int32)).cuda()
    want = ops.click_guide(tab, torch.from_numpy(p4).cuda(), cnt, out_hw, src, channels, stddev)
    for k in (4, 7, 64):
        pk = np.full((len(counts), 2, k, 2), 12345, np.int32)   # the slots past the counts are not read as clicks
        pk[:, :, :4] = p4
        got = ops.click_guide_list(tab, torch.from_numpy(pk).cuda(), cnt, out_hw, src, channels, stddev)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), k


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("stddev", [None, 5.0])
def test_guide_list_with_many_clicks_matches_float64(channels, stddev):
    """5, 20 and 64 clicks per kind, and a kind without clicks, within the bounds of DESIGN.md 7.3.5: Gaussian 2e-6,
    Euclidean 8 * 2^-24 * max(1, largest distance)."""
    from boxsegliver_amd import ops
    src, out_hw, k = (100, 104), (48, 56), 64
    counts = [(5, 20), (64, 0), (0, 64), (20, 5)]
    tab = _whole_slice_tab(len(counts), src)
    pts = np.full((len(counts), 2, k, 2), -1, np.int32)
    for j, c in enumerate(counts):
        for kind in range(2):
            pts[j, kind, :c[kind]] = _spread_clicks(c[kind], src, 5 * j + kind)
    got = ops.click_guide_list(tab, torch.from_numpy(pts).cuda(), torch.from_numpy(np.array(counts, np.int32)).cuda(), out_hw, src,
                               channels, stddev).cpu().numpy()
    for j, c in enumerate(counts):
        want, far = lits_inter_ref.sp_guide(src, out_hw, pts[j], c, (0, 0), stddev, channels)
        bound = 2e-6 if stddev is not None else 8 * 2.0 ** -24 * max(1.0, far)
        assert np.abs(got[j] - want).max() <= bound, (j, np.abs(got[j] - want).max(), bound)
        if channels == 2:
            for kind in range(2):
                if c[kind] == 0:
                    assert (got[j, ..., kind] == 0).all()


# ------------------------------------------------------------------------------------------------- the session loop
class _ToyPredictor(object):
    """The recorded sessions' predictor in place of the net: discs around the clicks, radii by slice; or a fixed mask."""

    def __init__(self, shape, by_slice):
        self.shape, self.by_slice = shape, by_slice

    def __call__(self, pts, cnt, slot_slices, fresh):
        p, c = pts.cpu().numpy(), cnt.cpu().numpy()
        out = np.zeros((len(slot_slices),) + tuple(self.shape), np.uint8)
        for j, s in enumerate(slot_slices):
            if s < 0:
                continue
            how = self.by_slice[s]
            if "pred" in how:
                out[j] = shapes.build(self.shape, how["pred"])
            else:
                out[j] = shapes.disc_prediction(self.shape, p[j, 0, :c[j, 0]], p[j, 1, :c[j, 1]], how["r_fg"], how["r_bg"])
        return torch.from_numpy(out).cuda()


@pytest.mark.parametrize("batch", [1, 2])
def test_recorded_sessions_through_the_session_loop(records, batch):
    """Click for click, counter for counter and stop reason for stop reason: the sessions the reference ran
    (make_inter_eval_fixtures.run_session) as the slices of one case per shape, the repeat session among them.  A recorded
    session was followed up to its first fallback round; there the loop must report a fallback click."""
    from boxsegliver_amd.entry import main_eval
    sessions = list(records["sessions"]) + [records["repeat"]]
    by_shape = {}
    for s in sessions:
        by_shape.setdefault(tuple(s["shape"]), []).append(s)
    seen_stops = set()
    for shape, group in by_shape.items():
        lb = torch.from_numpy(np.stack([shapes.build(shape, s["ref"]) for s in group]).astype(np.uint8) * LB_SCALE).cuda()
        vol = torch.zeros((len(group),) + shape, dtype=torch.uint8, device="cuda")
        trace = []
        inters = main_eval.run_case(lb, list(range(len(group))), _ToyPredictor(shape, group), shape, batch, group[0]["max_iter"],
                                    group[0]["inter_thresh"], 1, vol, 0, trace, "toy")
        total = [0, 0]
        for z, s in enumerate(group):
            mine = [r for r in trace if r[1] == z]
            n = [sum(1 for r in mine if r[2] is not None and r[3] == kind) for kind in range(2)]
            total[0], total[1] = total[0] + n[0], total[1] + n[1]
            for i, want in enumerate(s["rounds"]):
                assert list(mine[i][2]) == want["click"] and mine[i][3] == want["kind"] and not mine[i][4], (shape, z, i)
                assert list(mine[i + 1][5]) == want["counts"], (shape, z, i)                 # read with the next click
            last = mine[len(s["rounds"])]
            seen_stops.add(s["stop"])
            if s["stop"] == "fallback":
                assert last[4] and last[2] is not None, (shape, z)
            else:
                assert last[6] == s["stop"] and len(mine) == len(s["rounds"]) + 1 and n == s["num_iter"], (shape, z, last)
            assert mine[-1][6] is not None and all(r[6] is None for r in mine[:-1])
        assert inters == total
    assert seen_stops >= {"fallback", "repeat"}


# ------------------------------------------------------------------------------------------------- end to end
def _eval_argv(root, model, classes, batch, extra):
    argv = ("--mode eval --tag inter --model {} --classes {} --test_fold 1 --im_height 32 --im_width 32 --im_channel 3 "
            "--random_flip 3 --eval_mirror --batch_size {} --normalizer instance_norm --metrics_eval Dice VOE --max_iter 3 "
            "--inter_thresh 0.9").format(model, classes, batch).split()
    return argv + extra + ["--lits_root", str(root), "--model_dir", str(root / "run")]


@pytest.mark.parametrize("model,classes,batch,extra", [
    ("UNetInter", "Liver", 3, "--use_spatial --local_enhance --stddev 5."),
    ("UNetInter", "Liver", 1, "--use_spatial --local_enhance --stddev 5."),
    ("LGNet", "Tumor", 3, "--use_spatial --guide_channel 1"),
    ("UNet", "Liver", 3, ""),                                   # plain evaluation: one forward per object slice, no clicks
])
def test_main_eval_end_to_end_at_random_weights(tmp_path, model, classes, batch, extra):
    from boxsegliver_amd import loss_metrics
    from boxsegliver_amd.entry import main_eval
    cases = lits_inter_ref.write_dataset(tmp_path)
    args = main_eval.get_arguments(_eval_argv(tmp_path, model, classes, batch, extra.split()))
    assert main_eval.mirror_plan(args) == [0, 1, 2, 3]
    trace, volumes = [], {}
    results = main_eval.run(args, trace=trace, trace_preds=True, restore=False, volumes=volumes)
    obj = 1 if classes == "Liver" else 2
    assert sorted(volumes) == [2, 3]
    spatial = "--use_spatial" in extra
    per_metric = {"Dice": [], "VOE": []}
    tp = fp = fn = 0
    for pid, vol in volumes.items():
        label = (cases[pid][1] >= obj).astype(np.uint8)
        v = vol.cpu().numpy()
        assert v.shape == label.shape and v.dtype == np.uint8
        empty = ~label.any(axis=(1, 2))
        assert not v[empty].any()                                                         # slices without the object stay 0
        for key, value in loss_metrics.metric_3d(v, label, required=["Dice", "VOE"]).items():
            per_metric[key].append(value)
        tp, fp, fn = tp + int((v & label).sum()), fp + int((v & ~label & 1).sum()), fn + int((~v & label & 1).sum())
        mine = [r for r in trace if r[0] == pid]
        if not spatial:
            assert not mine
            continue
        assert sorted(set(r[1] for r in mine)) == np.nonzero(~empty)[0].tolist()           # every object slice is a session
        for z in set(r[1] for r in mine):
            rounds = [r for r in mine if r[1] == z]
            assert rounds[-1][6] in ("repeat", "dice", "max_iter", "empty") and all(r[6] is None for r in rounds[:-1])
            assert len([r for r in rounds if r[2] is not None]) <= 3
            assert not rounds[0][7].any()                                                  # round 0: all zeros
            for r in rounds:
                want = ref.click(shapes.resize_nearest(r[7], label.shape[1:]), label[z])
                assert r[5] == want["counts"], (pid, z)
                if r[2] is not None:
                    assert (r[2], r[3], r[4]) == (want["click"], want["kind"], want["fallback"]), (pid, z)
            np.testing.assert_array_equal(v[z], shapes.resize_nearest(rounds[-1][7], label.shape[1:]))   # the last forward's
    for key, values in per_metric.items():
        assert results["{}/{}".format(classes, key)] == pytest.approx(float(np.mean(values)), rel=1e-12, abs=1e-12)
    assert results["G_Dice"] == pytest.approx(2 * tp / (2 * tp + fn + fp) if tp + fn + fp else 0.0, rel=1e-12)
    if spatial:
        clicks = [sum(1 for r in trace if r[2] is not None and r[3] == kind) for kind in range(2)]
        assert (results["inters_fg"], results["inters_bg"]) == (clicks[0] / 2, clicks[1] / 2) and sum(clicks) >= len(set((r[0], r[1]) for r in trace))
        text = open(str(tmp_path / "run" / "logs" / "eval_inter")).read()
        assert "Evaluate-2 " in text and "(Num inters: [" in text and "---Infer 2 cases" in text and "(Average inters: " in text
    else:
        assert (results["inters_fg"], results["inters_bg"]) == (0.0, 0.0)


def test_main_and_main_g_still_refuse_liver_inter_eval(tmp_path):
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_g
    argv = ("liver_inter --mode eval --tag t --model UNetInter --classes Tumor --use_spatial --lits_root {} --model_dir {}".format(
        tmp_path, tmp_path / "run")).split()
    for main in (entry.main, main_g.main):
        with pytest.raises(NotImplementedError, match="offline evaluator"):
            main(argv)


def test_main_eval_scores_a_trained_checkpoint_from_the_command_line(tmp_path):
    """`main liver_inter` trains two steps; `main_eval` restores that checkpoint and scores it, the same way twice; without
    a checkpoint it raises FileNotFoundError."""
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval
    lits_inter_ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    common = ("--tag inter --model UNetInter --classes Tumor --test_fold 1 --im_height 32 --im_width 32 --im_channel 3 --random_flip 3 "
              "--batch_size 2 --normalizer instance_norm --use_spatial --local_enhance --stddev 5.").split() + \
        ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    argv_eval = ["--mode", "eval", "--max_iter", "2", "--metrics_eval", "Dice"] + common
    with pytest.raises(FileNotFoundError, match="Missing checkpoint"):
        main_eval.main(argv_eval)
    assert entry.main(["liver_inter", "--mode", "train", "--num_of_steps", "2", "--tumor_percent", "0.5", "--loss_weight_type",
                       "numerical", "--loss_numeric_w", "1", "1", "--learning_rate", "0.01", "--log_step", "1"] + common) == 0
    assert main_eval.main(argv_eval) == 0
    text = open(str(run / "logs" / "eval_inter")).read()
    assert "Evaluate-2 " in text and "Evaluate-3 " in text and "---Infer 2 cases - Tumor/Dice: " in text and " - G_Dice: " in text
    args = main_eval.get_arguments(argv_eval)
    first = []
    main_eval.run(args, trace=first, trace_preds=True)
    assert {r[0] for r in first} == {2, 3} and all(r[7].shape == (32, 32) for r in first)
    again = []
    main_eval.run(args, trace=again, trace_preds=True)
    assert all(np.array_equal(a[7], b[7]) and a[:7] == b[:7] for a, b in zip(first, again)) and len(again) == len(first)
