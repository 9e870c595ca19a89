"""GPU: the 3-D click guides of `liver_3d --use_spatial` (`unetk_lits3d_clicks`, `unetk_click_guide3d`; csrc/lits3d_clicks.hip;
DESIGN.md 7.3.6) against the restatement of the reference's 3-D pipeline (lits3d_clicks_ref.py, which cites the lines and
uses scipy's erosion with the reference's element literally) and against what the reference itself gave on the records of
tests/click3d_shapes.py; UNet3D with the guide among its input channels against the oracle; and `liver_3d --use_spatial`
training from the command line."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import click3d_shapes as c3
import guardbuf
import lits3d_clicks_ref as cref
import lits3d_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL, LARGE = (6, 16, 20), (6, 32, 40)        # test_gpu_lits3d.py's shapes: LARGE's 1.4 crop is clamped to the 40 x 48 slice
SMALL_CLICKS, REF_CLICKS, LAST = c3.SMALL_CLICKS, c3.REF_CLICKS, c3.LAST
# Gaussian guide: max |got - float64 restatement| over test_guide_matches_restatement's samples, measured on an MI355X (ROCm 7
# expf); asserted at four times that, to leave room for another compiler's expf.
GAUSS_MAX_DEV_MEASURED = 8.962e-8


@pytest.fixture(scope="module")
def store():
    cases = ref.make_cases()
    im, lb, base = ref.stack_store(cases)
    return dict(cases=cases, base=base, im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy(lb).cuda())


def _samples(shape, zoom):
    """(case, centre, crop, flips): corners and the interior of case 0, the tumour-free case 1, the shallow case 2, case 3."""
    from boxsegliver_amd.data import lits3d
    crop = tuple(int(v) for v in lits3d.crop_shape(shape[1:], [zoom, zoom * 0.97 + 0.03]))
    d0 = ref.DEPTHS[0]
    out = [(0, c, crop, (i & 1, (i >> 1) & 1, (i >> 2) & 1))
           for i, c in enumerate([(0, 0, 0), (d0 - 1, ref.H - 1, ref.W - 1), (0, ref.H - 1, 0), (d0 - 1, 0, ref.W - 1)])]
    out += [(0, (6, 19, 23), crop, (0, 0, 0)), (0, (7, 20, 22), crop, (1, 1, 1)), (1, (4, 20, 22), crop, (0, 0, 0)),
            (2, (2, 17, 21), crop, (0, 0, 0)), (2, (4, 39, 0), crop, (1, 0, 1)), (3, (5, 20, 40), crop, (0, 1, 0)),
            (3, (1, 17, 21), crop, (0, 0, 1))]
    return out


def _table(store, samples):
    rows = [ref.table_row(store["base"][ci], ref.DEPTHS[ci], c, crop, flips) for ci, c, crop, flips in samples]
    return torch.from_numpy(np.stack(rows)).cuda()


def _click_rows(n, seed):
    """uint32 [n, 12]: four clicks of each kind asked on most rows, both strategies, the draws 0 and LAST among them."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((n, 12), np.uint32)
    tab[:, 0] = 4
    tab[:, 1] = 4
    tab[:, 2] = np.where(np.arange(n) % 2 == 0, 1, 3)
    tab[:, 4:] = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    tab[0::3, 4], tab[1::3, 5], tab[1::3, 8], tab[0::3, 9] = 0, LAST, 0, LAST
    tab[2::5, 0], tab[3::5, 1], tab[4::7, 1] = 2, 0, 1
    return tab


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _run(lb, tab, rows, shape, params, obj_label=1):
    from boxsegliver_amd import ops
    ctab = torch.from_numpy(rows.view(np.int32)).cuda()
    status = _status()
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, obj_label, params)
    again = ops.lits3d_clicks(lb, tab, ctab, shape, status, obj_label, params)
    assert torch.equal(pts, again[0]) and torch.equal(cnt, again[1])                  # two calls give identical bits
    assert pts.shape == (tab.shape[0], 2, 4, 3) and cnt.shape == (tab.shape[0], 2) and pts.dtype == cnt.dtype == torch.int32
    return pts.cpu().numpy(), cnt.cpu().numpy(), int(status.item())


# ------------------------------------------------------------------------------------------------- clicks: the restatement
@pytest.mark.parametrize("shape,zoom", [(SMALL, 1.0), (SMALL, 1.25), (LARGE, 1.125), (LARGE, 1.4)])
@pytest.mark.parametrize("params", [SMALL_CLICKS, REF_CLICKS])
def test_clicks_equal_the_restatement(store, shape, zoom, params):
    samples = _samples(shape, zoom)
    tab = _table(store, samples)
    seen = dict(small=0, emptied=0, fg=0, bg=0, none=0, slices=0)
    for obj_label in (1, 2):
        rows = _click_rows(len(samples), 17 + obj_label)
        pts, cnt, status = _run(store["lb"], tab, rows, shape, params, obj_label)
        assert status == 0
        for j, (ci, c, crop, _) in enumerate(samples):
            obj, _ = cref.object_patch(store["cases"][ci][1], c, crop, shape, obj_label)
            trace = {}
            want_pts, want_cnt = cref.clicks(obj, rows[j].astype(np.uint64), params, trace)
            np.testing.assert_array_equal(cnt[j], want_cnt, err_msg=str((samples[j], obj_label)))
            np.testing.assert_array_equal(pts[j], want_pts, err_msg=str((samples[j], obj_label)))
            seen["fg"] += int(want_cnt[0])
            seen["bg"] += int(want_cnt[1])
            seen["none"] += int(not obj.any())
            seen["slices"] += int(len(set(want_pts[:, :, 0][want_pts[:, :, 0] >= 0].tolist())) > 1)
            for k in ("fg", "bg"):
                seen["small"] += int(trace[k].get("small", False))
                seen["emptied"] += int(trace[k].get("emptied", False))
    # every branch of the simulator ran (a kind that runs out of candidates: with the small parameters; the reference's
    # step of 10 clears these slices only in the records)
    assert all(v > 0 for k, v in seen.items() if k != "emptied" or params == SMALL_CLICKS), seen


# ------------------------------------------------------------------------------------------------- clicks: the records
def test_clicks_equal_the_reference_records():
    with open(os.path.join(HERE, "golden", "ref_clicks3d.json")) as f:
        fixture = json.load(f)
    groups = {}
    for rec in fixture["records"]:
        vol = c3.build(rec["volume"])
        want = fixture["volumes"][rec["volume"]]
        assert c3.checksum(vol) == (want["popcount"], want["index_sum"])
        groups.setdefault((rec["volume"], rec["depth"], tuple(rec["crop"]), tuple(rec["params"])), []).append(rec)
    deviations = 0
    for (vname, depth_out, crop, params), recs in groups.items():
        vol = c3.build(vname)
        lb = torch.from_numpy((vol * ref.LB_SCALE).astype(np.uint8)).cuda()
        tab = torch.from_numpy(np.stack([ref.table_row(0, vol.shape[0], r["centre"], crop) for r in recs])).cuda()
        rows = np.array([r["row"] for r in recs], dtype=np.uint64).astype(np.uint32)
        pts, cnt, status = _run(lb, tab, rows, (depth_out,) + crop, params)
        assert status == 0
        for j, rec in enumerate(recs):
            assert pts[j, 0, :cnt[j, 0]].tolist() == rec["fg"], (rec["id"], rec["row"][2])
            assert pts[j, 1, :cnt[j, 1]].tolist() == rec["bg"], (rec["id"], rec["row"][2])
            assert np.all(pts[j, 0, cnt[j, 0]:] == -1) and np.all(pts[j, 1, cnt[j, 1]:] == -1)
            deviations += int(bool(rec["raises"]))
    assert deviations == 2                                                            # the all-object patch, both rows


def test_strategy_3_on_a_patch_of_many_runs_per_thread():
    """16 x 100 x 104 voxels are ten 16-byte runs per thread of clk3_select_kernel: the arg-max skips runs by their bound
    against the thread's best so far, which the smaller patches (at most four runs per thread) barely reach.  Against the
    restatement, for first clicks on the first, a middle and the last slice that holds candidates."""
    vol = np.concatenate([c3.build("v100"), c3.build("v100")[::-1]])
    assert vol.shape == (16, 100, 104)
    shape, params = (16, 100, 104), REF_CLICKS
    lb = torch.from_numpy((vol * ref.LB_SCALE).astype(np.uint8)).cuda()
    rows = np.array([[4, 4, 3, 0, 0, LAST, 1 << 31, 12345, first, 0, 0, 0] for first in (0, 1 << 31, LAST, 3 << 29, 5 << 29)],
                    dtype=np.uint64).astype(np.uint32)
    tab = torch.from_numpy(np.stack([ref.table_row(0, 16, (8, 50, 52), shape[1:])] * len(rows))).cuda()
    pts, cnt, status = _run(lb, tab, rows, shape, params)
    assert status == 0
    obj, box = cref.object_patch(vol, (8, 50, 52), shape[1:], shape, 1)
    assert box == (0, 0, 0, 100, 104)
    dz_wins = 0
    for j in range(len(rows)):
        trace = {}
        want_pts, want_cnt = cref.clicks(obj, rows[j].astype(np.uint64), params, trace)
        np.testing.assert_array_equal(cnt[j], want_cnt)
        np.testing.assert_array_equal(pts[j], want_pts)
        assert want_cnt[1] == 4
        dz_wins += trace["bg"]["dz_wins"]
    assert dz_wins > 0


# ------------------------------------------------------------------------------------------------- clicks: guard bands
def test_clicks_guard_bands_and_bad_rows(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    samples = _samples(LARGE, 1.4)
    n = len(samples)
    tab = _table(store, samples)
    rows = _click_rows(n, 5)
    desc = ops.lits3d_clicks_desc(store["lb"], n, LARGE, 1, REF_CLICKS)
    nbytes = int(lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(desc)))
    assert nbytes > 0 and nbytes % 16 == 0
    want = ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(rows.view(np.int32)).cuda(), LARGE, _status(), 1, REF_CLICKS)

    def call(rows, ws_fill, ws_bytes=nbytes):
        ctab = guardbuf.guarded_input(torch.from_numpy(rows.view(np.float32)).cuda())
        pts, cnt, status = guardbuf.guarded((n, 2, 4, 3)), guardbuf.guarded((n, 2)), guardbuf.guarded((1,))
        status.view.view(torch.int32).zero_()
        status.snap = status.flat.clone()
        ws = guardbuf.GuardedWorkspace(nbytes)
        ws.fill(ws_fill)
        code = lib.unetk_lits3d_clicks(ctypes.byref(desc), _abi.ptr(store["lb"]), _abi.ptr(tab), ctypes.c_void_p(ctab.ptr()),
                                       ctypes.c_void_p(pts.ptr()), ctypes.c_void_p(cnt.ptr()), ctypes.c_void_p(status.ptr()),
                                       ctypes.c_void_p(ws.ptr()), ws_bytes, _abi.stream_ptr())
        torch.cuda.synchronize()
        assert ctab.check_untouched() and pts.check_untouched() and cnt.check_untouched() and status.check_untouched()
        assert ws.guard_intact()
        return code, pts, cnt, int(status.view.view(torch.int32).item())

    code, pts, cnt, status = call(rows, 0x00, nbytes - 1)
    assert code == -3 and pts.changed_anywhere() == 0 and cnt.changed_anywhere() == 0          # UNETK_E_WORKSPACE, nothing launched
    for fill in (0x00, 0xFF):                                                         # whatever the workspace held before
        code, pts, cnt, status = call(rows, fill)
        assert code == 0 and status == 0 and pts.unwritten() == 0 and cnt.unwritten() == 0
        assert torch.equal(pts.view.view(torch.int32), want[0]) and torch.equal(cnt.view.view(torch.int32), want[1])
    # rows of draws out of range: bit 2 (value 4), the values clamped, everything in bounds
    bad = rows.copy()
    bad[0, 0], bad[1, 0], bad[2, 1], bad[3, 2], bad[4, 2] = 0, 9, 0xFFFFFFFF, 0, 2
    clamped = bad.copy()
    clamped[0, 0], clamped[1, 0], clamped[2, 1], clamped[3, 2], clamped[4, 2] = 1, 4, 4, 1, 1
    code, pts, cnt, status = call(bad, 0xFF)
    assert code == 0 and status == 4
    ok = ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(clamped.view(np.int32)).cuda(), LARGE, _status(), 1, REF_CLICKS)
    assert torch.equal(pts.view.view(torch.int32), ok[0]) and torch.equal(cnt.view.view(torch.int32), ok[1])
    got = pts.view.view(torch.int32).cpu().numpy()
    assert got.min() >= -1 and got[..., 0].max() < LARGE[0] and got[..., 1].max() < ref.H and got[..., 2].max() < ref.W
    for k in range(5):                                                                # each bad value alone sets the bit
        one = rows.copy()
        one[k] = bad[k]
        assert call(one, 0x00)[3] == 4, k
    with pytest.raises(_abi.UnetkError, match="device tensors"):
        ops.lits3d_clicks(store["lb"].cpu(), tab.cpu(), torch.from_numpy(rows.view(np.int32)), LARGE, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_abi.UnetkError, match="unsupported"):
        ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(rows.view(np.int32)).cuda(), LARGE, _status(), 1, (3, 10, 252, 5))


# ------------------------------------------------------------------------------------------------- guide
def _guide_inputs(shape):
    samples = [(0, (6, 19, 23), shape[1:], (0, 0, 0)), (0, (6, 19, 23), (shape[1] + 6, shape[2] + 5), (1, 0, 1)),
               (0, (0, 1, 1), (shape[1] + 9, shape[2] + 9), (0, 1, 0)), (3, (2, 17, 21), (44, 60), (1, 1, 1)),
               (2, (3, 30, 30), (shape[1] + 1, shape[2] + 3), (1, 0, 0))]
    d = shape[0]
    pts = np.full((len(samples), 2, 4, 3), -1, np.int32)
    cnt = np.zeros((len(samples), 2), np.int32)
    pts[0, 0, :2], cnt[0] = [(0, 3, 4), (d - 1, 12, 17)], (2, 0)                      # no background click
    pts[1, 0, :1], pts[1, 1, :4], cnt[1] = [(2, 15, 16)], [(0, 0, 0), (d - 1, 21, 24), (1, 0, 24), (4, 21, 0)], (1, 4)
    pts[2, 1, :3], cnt[2] = [(1, 5, 5), (3, 6, 20), (5, 24, 28)], (0, 3)              # no foreground click
    pts[3, 0, :3], pts[3, 1, :1], cnt[3] = [(2, 20, 24), (3, 21, 24), (5, 39, 47)], [(0, 0, 47)], (3, 1)
    return samples, pts, cnt                                                          # sample 4: no click at all


@pytest.mark.parametrize("shape", [SMALL, LARGE])
@pytest.mark.parametrize("stddev", [None, (1.0, 3.0, 3.0), (2.0, 4.5, 2.5)])
def test_guide_matches_restatement(store, shape, stddev):
    """Euclidean: |got - ref| <= 8 * 2^-24 * max(1, largest distance) / normaliser (the squares are exact integers; the
    square root, the division and three lerps each round once).  Gaussian: measured, asserted at four times the measurement."""
    from boxsegliver_amd import ops
    samples, pts, cnt = _guide_inputs(shape)
    tab = _table(store, samples)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda()
    norm = cref.euclid_norm(shape[1])
    assert ops.click_guide3d_norm(shape[1]) == norm
    g2 = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 2, stddev)
    g1 = ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 1, stddev)
    assert g2.shape == (len(samples),) + shape + (2,) and g1.shape == (len(samples),) + shape + (1,) and g2.dtype == torch.float32
    assert torch.equal((g2[..., 0] - g2[..., 1]).view(torch.int32), g1[..., 0].view(torch.int32))     # G = 1 is fg - bg, bit for bit
    assert torch.equal(g2.view(torch.int32), ops.click_guide3d(tab, dp, dc, shape, (ref.H, ref.W), 2, stddev).view(torch.int32))
    got = g2.cpu().numpy()
    worst = 0.0
    for j, (ci, c, crop, flips) in enumerate(samples):
        box = ref.crop_box(c, crop, shape, ref.DEPTHS[ci], (ref.H, ref.W))
        want, far = cref.sp_guide((shape[0],) + box[3:], shape[1:], pts[j], cnt[j], flips, stddev, 2, norm)
        err = np.abs(got[j].astype(np.float64) - want).max()
        worst = max(worst, err)
        if stddev is None:
            tol = 8 * 2.0 ** -24 * max(1.0, far) / norm
            assert err <= tol, (j, err, tol)
        for kind in range(2):
            if cnt[j, kind] == 0:
                assert np.all(got[j][..., kind] == 0)                                 # a kind without clicks is exactly 0
            else:
                assert got[j][..., kind].max() > 0
    print("click_guide3d {} stddev {}: max |got - ref| = {:.3e}".format(shape, stddev, worst))
    if stddev is not None:
        assert worst <= 4 * GAUSS_MAX_DEV_MEASURED


def test_guide_flips_line_up_with_the_image(store):
    """A click on a marked voxel stays on it under all eight flips: crop = output, so crop voxels are output voxels."""
    from boxsegliver_amd import ops
    shape = (6, 16, 20)
    mark = (3, 21, 27)                                                                # (slice of the case, row, column)
    im = store["im"].clone()
    base = int(store["base"][3])
    im[base + mark[0], mark[1], mark[2]] = 32000                                      # brighter than any voxel of the case
    centre = (4, mark[1] + 2, mark[2] - 3)
    samples = [(3, centre, shape[1:], (i & 1, (i >> 1) & 1, (i >> 2) & 1)) for i in range(8)]
    z1, y1, x1, _, _ = ref.crop_box(centre, shape[1:], shape, ref.DEPTHS[3], (ref.H, ref.W))
    click = (mark[0] - z1, mark[1] - y1, mark[2] - x1)
    assert all(0 < click[a] < shape[a] - 1 for a in range(3)) and click[0] != shape[0] - 1 - click[0]
    pts = np.full((8, 2, 4, 3), -1, np.int32)
    pts[:, 0, 0] = click
    cnt = np.tile(np.array([[1, 0]], np.int32), (8, 1))
    tab = _table(store, samples)
    images = ops.lits_patch3d(im, store["lb"], tab, shape, False)[0][..., 0].cpu().numpy()
    seen = set()
    for stddev in ((1.0, 3.0, 3.0), None):
        g = ops.click_guide3d(tab, torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda(), shape, (ref.H, ref.W), 2,
                              stddev).cpu().numpy()[..., 0]
        for j in range(8):
            at = np.unravel_index(np.argmax(images[j]), shape)
            guide_at = np.unravel_index(np.argmax(g[j]) if stddev else np.argmin(g[j]), shape)
            assert at == guide_at, (j, at, guide_at)
            seen.add(at)
    assert len(seen) == 8                                                            # the eight flips are eight places


def test_guide_guard_bands(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    samples, pts, cnt = _guide_inputs(LARGE)
    n = len(samples)
    tab = _table(store, samples)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda()
    for g, stddev in ((2, (1.0, 3.0, 3.0)), (1, None)):
        desc = ops.lits3d_clicks_desc(store["lb"], n, LARGE, guide_channel=g, stddev=stddev, euclid_norm=cref.euclid_norm(LARGE[1]))
        out = guardbuf.guarded((n,) + LARGE + (g,))
        assert lib.unetk_click_guide3d(ctypes.byref(desc), _abi.ptr(tab), _abi.ptr(dp), _abi.ptr(dc), ctypes.c_void_p(out.ptr()),
                                       _abi.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert out.check_untouched() and out.unwritten() == 0
        want = ops.click_guide3d(tab, dp, dc, LARGE, (ref.H, ref.W), g, stddev)
        assert torch.equal(out.view.view(torch.int32), want.view(torch.int32))
    wild = dc.clone()
    wild[0, 0], wild[1, 1] = 99, -7                                                   # cnt is clamped into [0, 4]
    a = ops.click_guide3d(tab, dp, wild, LARGE, (ref.H, ref.W), 2, None)
    fixed = dc.clone()
    fixed[0, 0], fixed[1, 1] = 4, 0
    assert torch.equal(a.view(torch.int32), ops.click_guide3d(tab, dp, fixed, LARGE, (ref.H, ref.W), 2, None).view(torch.int32))


# ------------------------------------------------------------------------------------------------- the net
def _net_inputs(args, g):
    from boxsegliver_amd.data.synthetic import make_batch_3d
    images, labels, _ = make_batch_3d(2, args.im_depth, args.im_height, args.im_width, 1, 2, 1234)
    guide = np.random.default_rng(21).random(images.shape[:4] + (g,), dtype=np.float32)
    return images, labels, guide


@pytest.mark.parametrize("g", [1, 2])
def test_unet3d_with_the_guide_matches_the_oracle(g):
    """test_gpu_unet3d.py's parity check, its shape and its tolerances, with sp_guide among the input channels: the oracle is
    built with in_channels = 1 + G and fed the concatenated input."""
    from oracle import unet3d
    from boxsegliver_amd import ops
    from boxsegliver_amd.NetworksV2.UNet3D import UNet3D
    import test_gpu_unet3d as t3
    args = t3.make_args(use_spatial=True, guide_channel=g)
    images, labels, guide = _net_inputs(args, g)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda()}
    model = UNet3D(args)
    model(inputs, "eval", **t3.YML)
    net = unet3d.UNet3DOracle(1 + g, 2, normalizer=args.normalizer)
    assert [(n, tuple(s), k) for n, s, k in net.specs] == [(n, tuple(s), k) for n, s, k in model.params.logical_specs]
    assert dict((n, tuple(s)) for n, s, _ in net.specs)["UNet3D/conv_e0/conv1/weights"] == (1, 3, 3, 1 + g, 30)
    params = unet3d.init_params(net.specs, seed=5)
    gen = torch.Generator().manual_seed(9)
    for name, _, kind in net.specs:
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(params[name].shape, generator=gen)
        elif kind in ("beta", "bias"):
            params[name] = 0.1 * torch.randn(params[name].shape, generator=gen)
    model.params.load_state(params)
    x = torch.from_numpy(np.concatenate([images, guide], axis=-1))
    lab = torch.from_numpy(labels).long()
    total, _, logits, _, _ = net.loss_and_grads(params, x, lab, **t3.kwargs_of(args))
    p64 = {k: v.double() for k, v in params.items()}
    _, _, _, grads64, _ = net.loss_and_grads(p64, x.double(), lab, **t3.kwargs_of(args))
    ops.DEBUG_CAPTURE = []
    try:
        model.params.zero_grad()
        loss = model(inputs, "train", **t3.YML)
        loss.backward()
        torch.cuda.synchronize()
        captured = ops.DEBUG_CAPTURE
    finally:
        ops.DEBUG_CAPTURE = None
    assert abs(loss.item() - total.item()) < 1e-4 * max(1.0, abs(total.item()))
    got = model.layers["logits"].cpu().numpy()
    assert np.abs(got - logits.numpy()).max() < 1e-3
    convs = [c for c in captured if c["kind"] == "conv3d"]
    deconvs = [c for c in captured if c["kind"] == "deconv3d"]
    assert len(convs) == 18 and len(deconvs) == 4
    assert sorted(int(c["x"].shape[-1]) for c in convs)[0] == 1 + g                   # the first unit saw image + guide
    for c in convs:
        t3.check_conv3d_unit(c)                                                      # every unit's backward
    for c in deconvs:
        t3.check_deconv3d(c)
    num = den = 0.0
    for name in model.params.trainable_names():
        grad = model.params.logical_grad(name).numpy().astype(np.float64)
        want = grads64[name].numpy()
        num += np.sum((grad - want) ** 2)
        den += np.sum(want ** 2)
    assert (num / den) ** 0.5 < 1e-2
    first = model.params.logical_grad("UNet3D/conv_e0/conv1/weights").numpy()
    assert np.abs(first[..., 1:, :]).max() > 0                                        # the guide channels' filters get a gradient


def test_unet3d_bf16c_step_with_the_guide(monkeypatch):
    """One bf16c step with a two-channel guide against the float64 oracle of the same arithmetic: test_gpu_unet3d_bf16c.py's
    shape and bounds."""
    from oracle import tf_ops, unet3d
    from boxsegliver_amd.NetworksV2.UNet3D import UNet3D
    import test_gpu_unet3d_bf16c as tb
    args = tb.make_args(use_spatial=True, guide_channel=2)
    images, labels, guide = _net_inputs(args, 2)
    inputs = {"images": torch.from_numpy(images).cuda(), "labels": torch.from_numpy(labels).cuda(),
              "sp_guide": torch.from_numpy(guide).cuda()}
    model = UNet3D(args)
    model(inputs, "eval", **tb.YML)
    net = unet3d.UNet3DOracle(3, 2, normalizer=args.normalizer)
    params = tb._params(net)
    model.params.load_state(params)
    monkeypatch.setattr(tf_ops, "conv_nd_same", tb.bf16c_conv)
    monkeypatch.setattr(tf_ops, "conv_transpose_ks", tb.bf16c_conv_transpose)
    p64 = {k: v.double().cuda() for k, v in params.items()}
    x = torch.cat((inputs["images"], inputs["sp_guide"]), dim=-1).double()
    total, _, logits, grads, _ = net.loss_and_grads(
        p64, x, inputs["labels"].long(), loss_type=args.loss_type, loss_weight_type=args.loss_weight_type,
        numeric_w=args.loss_numeric_w, weight_decay_rate=args.weight_decay_rate)
    model.params.zero_grad()
    loss = model(inputs, "train", **tb.YML)
    loss.backward()
    torch.cuda.synchronize()
    got = model.layers["logits"].double()
    d = (got - logits).abs()
    agree = (got.argmax(-1) == logits.argmax(-1)).double().mean().item()
    gl2 = tb._grad_l2(model, grads)
    print("bf16c + guide: loss", abs(loss.item() - total.item()), "logits max", d.max().item(), "mean", d.mean().item(),
          "argmax", agree, "gradL2", gl2)
    assert abs(loss.item() - total.item()) < 1e-3 * max(1.0, abs(total.item()))
    assert d.max().item() < 5e-2 and d.mean().item() < 5e-3
    assert agree > 0.995
    assert gl2 < 0.1


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("extra,channels", [("--use_spatial --local_enhance", 2), ("--use_spatial --guide_channel 1", 1)])
def test_liver_3d_trains_with_click_guides_from_the_command_line(tmp_path, extra, channels):
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = ("liver_3d --mode train --tag cli3dg --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 4 --batches_per_epoch 2 --eval_num_batches_per_epoch 2 --eval_per_epoch --evaluator Volume "
            "--primary_metric Tumor/Dice --secondary_metric Liver/Dice --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --save_best --log_step 1").split()
    paths = ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    argv, argv_plain = argv + extra.split() + paths, argv + paths
    # the batches the run is fed
    args, _, _ = entry.get_arguments(argv)
    params = {"args": args, "lits_root": str(tmp_path)}
    gen = lits3d.input_fn("train", params)
    plain_args, _, _ = entry.get_arguments(argv_plain)
    plain = lits3d.input_fn("train", {"args": plain_args, "lits_root": str(tmp_path)})
    for step in range(4):
        feats, labels = next(gen)
        assert feats["images"].shape == (2, 4, 32, 32, 1) and labels.shape == (2, 4, 32, 32)
        guide = feats["sp_guide"]
        assert guide.shape == (2, 4, 32, 32, channels) and guide.dtype == torch.float32 and guide.is_cuda
        assert bool(torch.isfinite(guide).all())
        if channels == 2:
            assert 0.0 <= float(guide.min()) and float(guide.max()) <= 1.0            # the Gaussian
            assert float(guide[0, ..., 0].max()) > 0.5                                # the forced sample holds its object: a click
        if step == 0:                                                                # the first batch is the unguided run's
            pf, pl = next(plain)
            assert torch.equal(pf["images"], feats["images"]) and torch.equal(pl, labels) and "sp_guide" not in pf
    ev = [list(lits3d.input_fn("eval_online", params)) for _ in range(2)]
    assert len(ev[0]) == 2
    for (fa, la), (fb, lb) in zip(*ev):                                              # every evaluation sees the same clicks
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(fa["sp_guide"], fb["sp_guide"]) and torch.equal(la, lb)
    assert int(params[("lits3d_status", True)].item()) == 0 and int(params[("lits3d_status", False)].item()) == 0
    params[("lits3d_status", True)].fill_(4)
    with pytest.raises(RuntimeError, match="click draws"):
        next(lits3d.input_fn("eval_online", params))
    params[("lits3d_status", True)].zero_()
    # the command line
    assert entry.main(argv) == 0
    status = json.load(open(str(run / "checkpoint")))
    assert status["global_step"] == 4 and os.path.exists(str(run / status["model_checkpoint_path"]))
    losses = [float(v) for v in re.findall(r"loss = ([^,\s]+)", open(str(run / "logs" / "train_cli3dg")).read())]
    assert len(losses) >= 4 and all(np.isfinite(v) for v in losses)
    assert set(json.load(open(str(run / "best_result")))) == {"Liver/Dice", "Tumor/Dice"}
    argv_eval = [a for a in argv] + ["--eval_in_patches"]
    argv_eval[argv_eval.index("--mode") + 1] = "eval"
    with pytest.raises(NotImplementedError, match="--mode eval with --use_spatial"):
        entry.main(argv_eval)
