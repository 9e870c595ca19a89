"""GPU: the geodesic click guide (`unetk_lits_inter_center`, `unetk_click_geodesic`; csrc/lits_geodesic.hip) against its
restatement (lits_geodesic_ref.py: a heap Dijkstra in strict float32), through the C ABI in guarded buffers with the exact
workspace, then through `lits_inter.batches` and one `main_eval` session."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import guardbuf
import lits_geodesic_ref as ref
import lits_inter_ref

pytestmark = pytest.mark.gpu

SRC = (40, 48)                                 # the slices of lits3d_ref.make_cases
BIG = (1024, 1024)                             # a store extent that clamps none of the synthetic crops
K = 64


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


# ------------------------------------------------------------------------------------------------- through the C ABI
def _solve(base, pts, cnt, out_hw, crops, flips=None, channels=2, src_hw=BIG, want_dist=True):
    """unetk_click_geodesic in guarded buffers with the exact workspace, twice (sentinel and zero-filled workspace: identical
    bits).  base [N, hh, hw]; pts [N, 2, k, 2]; cnt [N, 2]; crops [N] of (ch, cw).  Returns (guide, dist, sweeps, path)."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    n, (h, w) = len(base), out_hw
    hh, hw = (h + 1) // 2, (w + 1) // 2
    flips = flips or [(0, 0)] * n
    tab = _i32(np.stack([lits_inter_ref.table_row(0, 1, (0, src_hw[0] // 2, src_hw[1] // 2), crops[j], (flips[j][0], flips[j][1], 0))
                         for j in range(n)]))
    desc = ops.click_geodesic_desc(n, out_hw, src_hw, channels)
    path = int(lib.unetk_click_geodesic_path(ctypes.byref(desc)))
    nbytes = int(lib.unetk_click_geodesic_ws_bytes(ctypes.byref(desc)))
    assert path in (1, 2) and nbytes > 0 and nbytes % 16 == 0
    d_base = guardbuf.guarded_input(torch.from_numpy(np.ascontiguousarray(base, np.float32)).cuda().reshape(n, hh, hw, 1))
    d_pts, d_cnt = _i32(pts), _i32(cnt)
    guide = guardbuf.guarded((n, h, w, channels))
    dist = guardbuf.guarded((n, 2, hh * hw, 1)) if want_dist else None
    status = _status()
    outs = []
    for fill in (None, 0):
        ws = guardbuf.GuardedWorkspace(nbytes)
        if fill is not None:
            ws.fill(fill)
        guide.reset()
        if dist is not None:
            dist.reset()
        args = (ctypes.byref(desc), _abi.ptr(tab), ctypes.c_void_p(d_base.ptr()), _abi.ptr(d_pts), _abi.ptr(d_cnt), int(pts.shape[2]),
                ctypes.c_void_p(guide.ptr()), ctypes.c_void_p(dist.ptr()) if dist is not None else None, _abi.ptr(status),
                ctypes.c_void_p(ws.ptr()))
        if fill is None:
            assert lib.unetk_click_geodesic(*args, nbytes - 1, _abi.stream_ptr()) == -3              # a workspace one byte short
            torch.cuda.synchronize()
            assert guide.changed_anywhere() == 0
        assert lib.unetk_click_geodesic(*args, nbytes, _abi.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert ws.guard_intact() and guide.check_untouched() and guide.unwritten() == 0 and d_base.changed_anywhere() == 0
        assert dist is None or (dist.check_untouched() and dist.unwritten() == 0)
        assert int(status.item()) == 0
        sweeps = ws.buf[ws.off:ws.off + n * 8].clone().view(torch.int32).view(n, 2).cpu().numpy()
        outs.append((guide.view.clone(), dist.view.clone() if dist is not None else None, sweeps))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))                    # two calls, identical bits
    if dist is not None:
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    g, d, sweeps = outs[0]
    return g.cpu().numpy(), d.cpu().numpy().reshape(n, 2, hh, hw) if d is not None else None, sweeps, path


def _clicks(seed_lists, k=K):
    """pts [N, 2, k, 2], cnt [N, 2] and the crop factor: on a crop of (2H, 2W) the click 4 g + 1 maps to g + 1/4 before the
    truncation, safely inside cell g.  Slots past the counts hold values no click may be read from."""
    n = len(seed_lists)
    pts = np.full((n, 2, k, 2), 0x7FFFFFF0, np.int32)
    cnt = np.zeros((n, 2), np.int32)
    for j, kinds in enumerate(seed_lists):
        for kind, seeds in enumerate(kinds):
            cnt[j, kind] = len(seeds)
            for i, (gy, gx) in enumerate(seeds):
                pts[j, kind, i] = (4 * gy + 1, 4 * gx + 1)
    return pts, cnt


def _out_of(grid):
    return 2 * grid[0] - 1, 2 * grid[1] - 1                     # odd H, W: hh = grid


def _check_dist(dist, base, seed_lists, pts, cnt, out_hw, crop):
    for j, kinds in enumerate(seed_lists):
        for kind, seeds in enumerate(kinds):
            assert ref.seeds_of(pts[j, kind], cnt[j, kind], crop, out_hw) == list(seeds)              # the clicks mean these seeds
            want = ref.dijkstra(base[j], list(seeds))
            np.testing.assert_array_equal(dist[j, kind].view(np.int32), want.view(np.int32), err_msg=str((j, kind)))


@pytest.mark.parametrize("grid", [(1, 1), (1, 5), (5, 1), (5, 4), (8, 8), (37, 23)])
def test_solve_equals_the_restatement(grid):
    """One seed, four seeds in the corners, 64 with duplicates, one kind empty, both kinds empty -- bit for bit."""
    hh, hw = grid
    rng = np.random.default_rng(7 * hh + hw)
    corners = [(0, 0), (0, hw - 1), (hh - 1, 0), (hh - 1, hw - 1)]
    many = [(int(rng.integers(0, hh)), int(rng.integers(0, hw))) for _ in range(20)]
    many = (many + many + many + corners)[:64]
    four = [(int(rng.integers(0, hh)), int(rng.integers(0, hw))) for _ in range(4)]
    base = np.stack([ref.field_normal(hh, hw, seed=hh * hw), ref.field_step(hh, hw), ref.field_constant(hh, hw),
                     ref.field_normal(hh, hw, seed=1 + hh * hw)])
    seed_lists = [([(hh // 2, hw // 3)], corners), (many, []), ([], four), ([], [])]
    out_hw = _out_of(grid)
    crop = (2 * out_hw[0], 2 * out_hw[1])
    pts, cnt = _clicks(seed_lists)
    guide, dist, sweeps, path = _solve(base, pts, cnt, out_hw, [crop] * 4)
    assert path == 1
    _check_dist(dist, base, seed_lists, pts, cnt, out_hw, crop)
    assert not dist[1, 1].any() and not dist[2, 0].any() and not dist[3].any()                        # false_fn: exactly 0
    assert not guide[1, ..., 1].any() and not guide[2, ..., 0].any() and not guide[3].any()
    assert sweeps[3].tolist() == [0, 0] and sweeps[0].min() >= 1
    assert sweeps.max() <= hh * hw                                                                    # the bound, never reached (status 0)
    np.testing.assert_array_equal(np.ascontiguousarray(guide[:, ::2, ::2, :]).view(np.int32),           # odd H, W, no flips
                                  np.ascontiguousarray(np.moveaxis(dist, 1, -1)).view(np.int32))


def test_maze_needs_and_gets_more_sweeps_than_a_fixed_count():
    """The 33 x 33 spiral of the host test: the corridor is followed to the centre, which a sweep count tied to the grid's
    extent cannot do (tests/test_lits_geodesic_host.py asserts a Jacobi needs more than 4 * 33)."""
    maze = ref.field_maze(33)
    seed_lists = [([(0, 0)], [(0, 0), (32, 0)])]
    out_hw = _out_of((33, 33))
    crop = (2 * out_hw[0], 2 * out_hw[1])
    pts, cnt = _clicks(seed_lists, k=4)
    guide, dist, sweeps, path = _solve(maze[None], pts, cnt, out_hw, [crop])
    _check_dist(dist, maze[None], seed_lists, pts, cnt, out_hw, crop)
    assert dist[0, 0][maze == 0].max() > 4 * 33 and dist[0, 0][maze == 0].max() < 1000
    print("maze sweeps", sweeps.tolist())


@pytest.mark.parametrize("out_hw", [(9, 7), (16, 16)])
def test_guide_resize_flips_and_channels(out_hw):
    """Odd H, W: the align-corners scale is exactly 1/2, so the guide at even pixels IS the distance, under all four flips.
    Everywhere (and for even H, W): the float64 resize of the distances within the bound test_gpu_lits_inter.py applies to
    unetk_click_guide's resize, 8 * 2^-24 * max(1, largest distance).  G = 1 is fg - bg of G = 2, bit for bit."""
    hh, hw = (out_hw[0] + 1) // 2, (out_hw[1] + 1) // 2
    flips = [(0, 0), (1, 0), (0, 1), (1, 1)]
    base = np.stack([ref.field_normal(hh, hw, seed=11)] * 4)
    crop = (30, 45)                                             # a crop above the output: several clicks share a cell
    pts = np.full((4, 2, 4, 2), -1, np.int32)
    pts[:, 0, :2] = [(3, 4), (29, 44)]
    pts[:, 1, :3] = [(0, 44), (15, 20), (16, 21)]
    cnt = np.tile(np.array([[2, 3]], np.int32), (4, 1))
    g2, dist, _, _ = _solve(base, pts, cnt, out_hw, [crop] * 4, flips)
    g1, _, _, _ = _solve(base, pts, cnt, out_hw, [crop] * 4, flips, channels=1, want_dist=False)
    np.testing.assert_array_equal((g2[..., 0] - g2[..., 1]).view(np.int32), g1[..., 0].view(np.int32))
    for j, f in enumerate(flips):
        want, want_dist = ref.guide(base[j], pts[j], cnt[j], crop, out_hw, f)
        np.testing.assert_array_equal(dist[j].view(np.int32), want_dist.view(np.int32))
        tol = 8 * 2.0 ** -24 * max(1.0, float(want_dist.max()))
        err = np.abs(g2[j].astype(np.float64) - want).max()
        assert err <= tol, (j, err, tol)
        if out_hw[0] % 2 == 1 and out_hw[1] % 2 == 1:
            back = g2[j][::-1] if f[1] else g2[j]
            back = back[:, ::-1] if f[0] else back
            np.testing.assert_array_equal(np.ascontiguousarray(back[::2, ::2]).view(np.int32),
                                          np.ascontiguousarray(np.moveaxis(dist[j], 0, -1)).view(np.int32))
    assert len({g2[j].tobytes() for j in range(4)}) == 4                                             # four flips, four guides


@pytest.mark.parametrize("grid,want_path", [((128, 128), 1), ((192, 160), 2)])
def test_both_paths_equal_the_restatement(grid, want_path):
    """The 256^2 training shape in LDS, a larger grid in the workspace: a random field, four seeds per kind."""
    hh, hw = grid
    rng = np.random.default_rng(hh)
    base = ref.field_normal(hh, hw, seed=hh + hw)[None]
    seed_lists = [([(int(rng.integers(0, hh)), int(rng.integers(0, hw))) for _ in range(4)],
                   [(0, 0), (hh - 1, hw - 1), (int(rng.integers(0, hh)), int(rng.integers(0, hw))), (hh // 2, hw // 2)])]
    out_hw = (2 * hh, 2 * hw)                                   # even: hh = H / 2
    crop = (2 * out_hw[0], 2 * out_hw[1])
    pts, cnt = _clicks(seed_lists, k=4)
    guide, dist, sweeps, path = _solve(base, pts, cnt, out_hw, [crop])
    assert path == want_path
    _check_dist(dist, base, seed_lists, pts, cnt, out_hw, crop)
    print("grid {} path {} sweeps {}".format(grid, path, sweeps.tolist()))


def test_a_grid_above_the_limit_is_refused():
    from boxsegliver_amd import _abi, ops
    assert ops.click_geodesic_path((1024, 1024)) == 2 and ops.click_geodesic_path((256, 256)) == 1
    assert ops.click_geodesic_path((1026, 1026)) == 0                                                # 513^2 > 2^18
    desc = ops.click_geodesic_desc(1, (1026, 1026), BIG)
    assert int(_abi.lib().unetk_click_geodesic_ws_bytes(ctypes.byref(desc))) == 0
    tab = _i32(np.stack([lits_inter_ref.table_row(0, 1, (0, 5, 5), (10, 10))]))
    one = torch.zeros(4, dtype=torch.int32, device="cuda")
    f = torch.zeros(16, dtype=torch.float32, device="cuda")
    rc = _abi.lib().unetk_click_geodesic(ctypes.byref(desc), _abi.ptr(tab), _abi.ptr(f), _abi.ptr(one), _abi.ptr(one), 1, _abi.ptr(f),
                                         None, _abi.ptr(one), _abi.ptr(f), 64, _abi.stream_ptr())
    assert rc == -2                                                                                  # UNETK_E_UNSUPPORTED, nothing launched
    with pytest.raises(_abi.UnetkError, match="unsupported output"):
        ops.click_geodesic(tab, torch.zeros((1, 513, 513), device="cuda"), torch.zeros((1, 2, 1, 2), dtype=torch.int32, device="cuda"),
                           torch.zeros((1, 2), dtype=torch.int32, device="cuda"), (1026, 1026))


# ------------------------------------------------------------------------------------------------- the base field
@pytest.fixture(scope="module")
def store():
    rng = np.random.default_rng(5)
    dark = np.zeros((3,) + SRC, np.uint16)                      # a case whose left half is zero: an all-zero crop
    dark[:, :, 30:] = 1000 + rng.integers(0, 3000, (3, SRC[0], 18))
    cases = lits_inter_ref.make_cases() + [(dark, np.zeros((3,) + SRC, np.uint8))]
    im, lb, base = lits_inter_ref.stack_store(cases)
    return dict(cases=cases, base=base, im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy(lb).cuda())


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("out_hw", [(9, 7), (16, 16)])
def test_centre_field_is_the_batch_at_every_second_pixel(store, c, out_hw):
    """Bit-equal to lits_inter_batch(training=False)[:, ::2, ::2, C // 2] on the table with the flips cleared: a crop below and
    one above the output, one clamped by the slice, centre slices at both ends of the case, an all-zero crop.  The flip
    columns change nothing."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    depth0 = store["cases"][0][0].shape[0]
    dark = len(store["cases"]) - 1
    samples = [(0, (6, 19, 23), (7, 5)), (0, (6, 19, 23), (33, 37)), (0, (6, 2, 45), (44, 60)), (0, (0, 20, 20), (24, 28)),
               (0, (depth0 - 1, 20, 20), (24, 28)), (dark, (1, 20, 10), (12, 14)), (dark, (1, 20, 34), out_hw)]
    n = len(samples)

    def table(flips):
        return _i32(np.stack([lits_inter_ref.table_row(store["base"][ci], store["cases"][ci][0].shape[0], ctr, crop, flips[j] + (0,))
                              for j, (ci, ctr, crop) in enumerate(samples)]))

    plain = table([(0, 0)] * n)
    flipped = table([(j & 1, (j >> 1) & 1) for j in range(1, n + 1)])
    shape = (c,) + out_hw
    hh, hw = (out_hw[0] + 1) // 2, (out_hw[1] + 1) // 2
    status = _status()
    images, _ = ops.lits_inter_batch(store["im"], store["lb"], plain, shape, False, status)
    want = images[:, ::2, ::2, c // 2].contiguous()
    assert want.shape == (n, hh, hw) and not want[5].any() and want[:5].abs().max() > 0 and want[6].abs().max() > 0
    desc = ops.lits_inter_desc(store["im"], n, shape)
    nbytes = int(lib.unetk_lits_inter_center_ws_bytes(ctypes.byref(desc)))
    assert nbytes > 0 and nbytes % 16 == 0
    for tab in (plain, flipped):
        for fill in (0x00, 0xFF):
            out, ws = guardbuf.guarded((n, hh * hw, 1)), guardbuf.GuardedWorkspace(nbytes)
            ws.fill(fill)
            args = (ctypes.byref(desc), _abi.ptr(store["im"]), _abi.ptr(tab), ctypes.c_void_p(out.ptr()), _abi.ptr(status),
                    ctypes.c_void_p(ws.ptr()))
            assert lib.unetk_lits_inter_center(*args, nbytes - 1, _abi.stream_ptr()) == -3
            assert lib.unetk_lits_inter_center(*args, nbytes, _abi.stream_ptr()) == 0
            torch.cuda.synchronize()
            assert ws.guard_intact() and out.check_untouched() and out.unwritten() == 0
            assert torch.equal(out.view.reshape(n, hh, hw).view(torch.int32), want.view(torch.int32))
    assert torch.equal(ops.lits_inter_center(store["im"], flipped, shape, status).view(torch.int32), want.view(torch.int32))
    assert int(status.item()) == 0
    # a centre slice outside its case: zeros and bit 1, as unetk_lits_inter_batch reports it
    bad = _i32(np.stack([lits_inter_ref.table_row(store["base"][0], depth0, (depth0 + 3, 19, 23), (24, 28))]))
    assert not ops.lits_inter_center(store["im"], bad, shape, status).any() and int(status.item()) == 2
    with pytest.raises(_abi.UnetkError, match="unsupported shape"):
        ops.lits_inter_center(store["im"], plain, (2,) + out_hw, status)


# ------------------------------------------------------------------------------------------------- the pipeline
def _pipeline(tmp_path, extra=()):
    from boxsegliver_amd.data import lits_inter
    from boxsegliver_amd.entry import main as entry
    argv = ("liver_inter --mode train --tag geo --model UNetInter --classes Tumor --test_fold 1 --im_height 33 --im_width 33 "
            "--im_channel 3 --random_flip 3 --noise_scale 0.05 --tumor_percent 0.5 --batch_size 2 --use_spatial --geodesic_guide "
            "--local_enhance --stddev 5.").split() + list(extra) + ["--lits_root", str(tmp_path), "--model_dir", str(tmp_path / "run")]
    args, _, _ = entry.get_arguments(argv, guided=True)
    params = {"args": args, "lits_root": str(tmp_path)}
    return lits_inter, args, params


def test_batches_render_the_geodesic_guide(tmp_path):
    """`lits_inter.batches` with --geodesic_guide on the synthetic dataset of the existing tests, H = W = 33: the guide is
    click_geodesic of the batch's own table and clicks, exactly 0 on every mapped seed at its flipped place in the image, and
    two generators with one seed give identical bits."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits, lits3d
    lits_inter_ref.write_dataset(tmp_path)
    lits_inter, args, params = _pipeline(tmp_path)
    obj = lits_inter.check_args(args)
    first = next(lits_inter.input_fn("train", params))                                               # builds the store and the counts
    store, cases = params[("lits_store", True)]
    shape = (3, 33, 33)

    def sampler():
        return lits3d.PatchSampler(cases, store.offset, params[("lits3d_counts", True, obj)], 2, shape, store.im.shape[1:],
                                   tumor_percent=0.5, zoom_scale=args.zoom_scale, random_flip=3, training=True, seed=1234)

    status = _status()
    feats, labels = next(lits_inter.batches(store, sampler(), args, obj, status))
    again, _ = next(lits_inter.batches(store, sampler(), args, obj, status))
    assert feats["sp_guide"].shape == (2, 33, 33, 2) and feats["sp_guide"].dtype == torch.float32 and feats["sp_guide"].is_cuda
    assert torch.equal(feats["sp_guide"].view(torch.int32), again["sp_guide"].view(torch.int32))
    assert torch.equal(feats["sp_guide"].view(torch.int32), first[0]["sp_guide"].view(torch.int32))   # input_fn's own first batch
    assert torch.equal(feats["images"].view(torch.int32), again["images"].view(torch.int32))
    # the same draws by hand
    s = sampler()
    b = s.draw()
    clicks = lits_inter.draw_click_tab(s.rng, s.bs)
    tab, ctab = lits.upload_pinned([s.table(b), clicks.view(np.int32)], store.device)
    if s.force:
        ops.lits_pick_voxels(store.lb, tab, obj, status, lits.LB_SCALE)
    pts, cnt = ops.lits_clicks(store.lb, tab, ctab, status, obj, lits_inter.CLICKS, lits.LB_SCALE)
    base = ops.lits_inter_center(store.im, tab, shape, status, lits.IM_SCALE)
    want, dist = ops.click_geodesic(tab, base, pts, cnt, (33, 33), 2, want_dist=True, status=status, src_hw=store.im.shape[1:])
    assert torch.equal(feats["sp_guide"].view(torch.int32), want.view(torch.int32))
    assert int(status.item()) == 0
    g, t, p, c = feats["sp_guide"].cpu().numpy(), tab.cpu().numpy(), pts.cpu().numpy(), cnt.cpu().numpy()
    fields, dists = base.cpu().numpy(), dist.cpu().numpy()
    seen = 0
    for j in range(2):
        crop = (min(max(int(t[j, 5]), 1), SRC[0]), min(max(int(t[j, 6]), 1), SRC[1]))
        for kind in range(2):
            seeds = ref.seeds_of(p[j, kind], c[j, kind], crop, (33, 33))
            np.testing.assert_array_equal(dists[j, kind].view(np.int32), ref.dijkstra(fields[j], seeds).view(np.int32))
            for gy, gx in seeds:
                y, x = 2 * gy, 2 * gx
                y, x = (32 - y if t[j, 8] else y), (32 - x if t[j, 7] else x)
                assert g[j, y, x, kind] == 0
                seen += 1
            if not seeds:
                assert not g[j, ..., kind].any()
            else:
                assert (dists[j, kind] == 0).sum() == len(set(seeds))                                 # c >= 1: only the seeds are at 0
    assert seen >= 2


# ------------------------------------------------------------------------------------------------- evaluation
class _StubNet(object):
    """In place of the net: the object is where the foreground guide is below 5; keeps every guide it was handed."""
    params = ()

    def __init__(self):
        self.guides = []

    def __call__(self, feats, mode, *args, **kwargs):
        g = feats["sp_guide"]
        self.guides.append(g.clone())
        fg = (g[..., 0] < 5.0).float()
        self.probability = torch.stack([1 - fg, fg], dim=-1).contiguous()


def test_one_main_eval_session_feeds_the_geodesic_guide():
    """One session on a 32 x 32 case: the guide the net gets in round r is click_geodesic of the click lists after r clicks,
    on the base field of the whole slice; the session ends by a recorded stop reason."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.entry import main_eval
    rng = np.random.default_rng(9)
    im = (2000 + rng.integers(0, 2000, (3, 32, 32))).astype(np.uint16)
    lab = np.zeros((3, 32, 32), np.uint8)
    lab[1, 6:20, 8:26] = 2
    im[1][lab[1] > 0] += 6000
    store = argparse.Namespace(im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy((lab * lits.LB_SCALE).astype(np.uint8)).cuda(),
                               device=torch.device("cuda", torch.cuda.current_device()))
    args = main_eval.get_arguments("--mode eval --tag t --model UNetInter --classes Tumor --im_height 32 --im_width 32 --im_channel 3 "
                                   "--use_spatial --geodesic_guide --max_iter 4 --inter_thresh 0.95 --batch_size 1".split())
    assert main_eval.check_args(args) == 2
    stub = _StubNet()
    net = main_eval.NetPredictor(stub, (), {}, store, args, 2)
    net.case = (0, 3)
    lists = []

    def predict(pts, cnt, slot_slices, fresh):
        lists.append((pts.clone(), cnt.clone()))
        return net(pts, cnt, slot_slices, fresh)

    vol = torch.zeros((3, 32, 32), dtype=torch.uint8, device="cuda")
    trace = []
    inters = main_eval.run_case(store.lb, [1], predict, (32, 32), 1, 4, 0.95, 2, vol, 0, trace, "toy")
    assert trace[-1][6] in ("repeat", "dice", "max_iter", "empty") and all(r[6] is None for r in trace[:-1])
    assert len(stub.guides) == len(lists) >= 1 and sum(inters) >= len(lists)
    base = ops.lits_inter_center(store.im, net.tab, (3, 32, 32), net.status, lits.IM_SCALE)
    assert torch.equal(base.view(torch.int32), net.base.view(torch.int32))
    images, _ = ops.lits_inter_batch(store.im, store.lb, net.tab, (3, 32, 32), False, net.status, 2)
    assert torch.equal(base.view(torch.int32), images[:, ::2, ::2, 1].contiguous().view(torch.int32))
    for r, ((pts, cnt), got) in enumerate(zip(lists, stub.guides)):
        assert int(cnt.sum()) == r + 1 and tuple(pts.shape) == (1, 2, 4, 2)                           # one more click every round
        want = ops.click_geodesic(net.tab, base, pts, cnt, (32, 32), 2, src_hw=(32, 32))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), r
        assert got.shape == (1, 32, 32, 2) and bool(torch.isfinite(got).all())
    assert int(net.status.item()) == 0
