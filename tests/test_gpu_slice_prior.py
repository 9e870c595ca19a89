"""GPU: the slice prior of click-guided UNet3D (`unetk_slice_prior_field`, `unetk_slice_prior_render`; csrc/slice_prior.hip;
DESIGN.md 7.3.11) through the C ABI, in guarded buffers, against the restatement of the reference (slice_prior_ref.py: the
reference's own scipy transform of the 3-D array with one seeded slice); then `liver_3d --slice_prior` batches, one training
step of UNet3D on them, and `main_eval_3d --slice_prior` end to end.

Bounds of the render (set before any run): with H, W == ch, cw the resize is the identity and channel 1 is expf(-sqrtf(n) / 25)
for an exact integer n: the argument d / 25 carries at most about 1.5 ulp, x e^-x <= 1 / e, HIP's expf is documented at 1 ulp
and the values are at most 1, so the error stays under 4 * 2^-24 < 5e-7 absolute.  A real resize adds three lerps' roundings
of values at most 1: 1e-6.  Measured on an MI355X, 2026-10-21: at most 5.0e-8 at the identity resize and 9.9e-8 with a resize
(the tests print every row's figure before they assert)."""
import ctypes

import numpy as np
import pytest
import torch

import guardbuf
import lits3d_ref as ref
import slice_prior_ref as sref

pytestmark = pytest.mark.gpu

IDENTITY_TOL, RESIZE_TOL = 5e-7, 1e-6
STAGE = 128                                     # IEDT_STAGE of csrc/edt_int.h: rows of a strip staged at a time
SRC_A = (40, 80)
D = 4


# ------------------------------------------------------------------------------------------------- stores
def _store_a():
    """Two cases on 40 x 80 slices, labels in {0, 1, 2}: case 0 (12 slices) holds one pattern per slice, case 1 (3 slices) is
    shallower than D."""
    h, w = SRC_A
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    c0 = np.zeros((12, h, w), np.uint8)
    c0[0][((yy - 19) / 13.0) ** 2 + ((xx - 37) / 30.0) ** 2 <= 1] = 1
    c0[0][((yy - 17) / 5.0) ** 2 + ((xx - 30) / 9.0) ** 2 <= 1] = 2
    c0[1][20, 41] = 2                                                            # a single-pixel object
    c0[2][:] = 1                                                                 # fills every box (label 1), no tumour
    c0[3][(np.abs(yy - 20) <= 2) | (np.abs(xx - 40) <= 2)] = 2                   # a cross: touches all four borders of a box
    c0[4][rng.random((h, w)) < 0.4] = 2
    c0[5][((yy - 22) / 9.0) ** 2 + ((xx - 48) / 21.0) ** 2 <= 1] = 2
    for z in range(6, 12):
        c0[z][((yy - 15 - z) / 8.0) ** 2 + ((xx - 20 - 3 * z) / 14.0) ** 2 <= 1] = 1 + (z % 2)
    c1 = np.zeros((3, h, w), np.uint8)
    c1[:, 5:30, 10:70] = 1
    c1[1, 8:20, 30:52] = 2
    c1[2][rng.random((h, w)) < 0.1] = 2
    return [c0, c1]


def _store_b():
    """One case on 130 x 260 slices: a box one row past the column staging length and one column past a row block's 256."""
    rng = np.random.default_rng(4)
    lab = np.zeros((2, 130, 260), np.uint8)
    yy, xx = np.meshgrid(np.arange(130), np.arange(260), indexing="ij")
    lab[0][((yy - 70) / 50.0) ** 2 + ((xx - 120) / 110.0) ** 2 <= 1] = 1
    lab[0][129, 259] = 1                                                         # the last staged row / the second row block
    lab[1][rng.random((130, 260)) < 0.003] = 1
    return [lab]


class Store(object):
    def __init__(self, cases, seed=0):
        self.cases = cases
        self.base = np.concatenate(([0], np.cumsum([c.shape[0] for c in cases])))[:-1]
        lb = np.concatenate([(c * ref.LB_SCALE).astype(np.uint8) for c in cases])
        rng = np.random.default_rng(seed)
        im = (rng.random(lb.shape) * 450 * ref.IM_SCALE).astype(np.uint16)
        im[:, :3] = 0                                                            # air: the z-score's mask has a border
        self.im_np = im
        self.lb = torch.from_numpy(lb).cuda()
        self.im = torch.from_numpy(im.view(np.int16)).cuda()
        self.src = lb.shape[1:]

    def row(self, ci, centre, crop, flips=(0, 0, 0)):
        return ref.table_row(self.base[ci], self.cases[ci].shape[0], centre, crop, flips)


@pytest.fixture(scope="module")
def store_a():
    return Store(_store_a())


@pytest.fixture(scope="module")
def store_b():
    return Store(_store_b())


# ------------------------------------------------------------------------------------------------- the C ABI, guarded
def _desc(store, n, shape, obj):
    from boxsegliver_amd import ops
    return ops.lits3d_clicks_desc(store.lb, n, shape, obj)


def _field(store, tab, pts, cnt, shape, obj, mode, whole, boxes):
    """unetk_slice_prior_field in guarded buffers -> (field int32 [N, plane], z0 int32 [N]).  boxes: (bh, bw) per row -- exactly
    the box is written, nothing else of the plane, nothing outside it, and the workspace's guard stays intact."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    n, plane = tab.shape[0], store.src[0] * store.src[1]
    desc = _desc(store, n, shape, obj)
    k = 0 if pts.dim() == 4 else int(pts.shape[1])
    nbytes = int(lib.unetk_slice_prior_ws_bytes(ctypes.byref(desc)))
    assert nbytes == n * plane * 4
    out = guardbuf.guarded((n, plane))
    z0 = guardbuf.guarded((n, 1))
    ws = guardbuf.GuardedWorkspace(nbytes)
    results = []
    for _ in range(2):                                                           # two calls give identical bits
        out.reset()
        z0.reset()
        code = lib.unetk_slice_prior_field(ctypes.byref(desc), _abi.ptr(store.lb), _abi.ptr(tab), _abi.ptr(pts), _abi.ptr(cnt), k,
                                           1 if whole else 0, ops.SLICE_PRIOR_MODES[mode], ctypes.c_void_p(out.ptr()),
                                           ctypes.c_void_p(z0.ptr()), ctypes.c_void_p(ws.ptr()), nbytes, _abi.stream_ptr())
        assert code == 0, code
        torch.cuda.synchronize()
        results.append((out.view.clone().view(torch.int32).cpu().numpy(), z0.view.clone().view(torch.int32).cpu().numpy()[:, 0]))
    assert out.check_untouched() and z0.check_untouched() and ws.guard_intact() and z0.unwritten() == 0
    assert out.unwritten() == sum(plane - bh * bw for bh, bw in boxes)
    sent = np.int32(guardbuf.SENTINEL[torch.float32])
    for j, (bh, bw) in enumerate(boxes):
        assert not (results[0][0][j, :bh * bw] == sent).any() and (results[0][0][j, bh * bw:] == sent).all()
    np.testing.assert_array_equal(results[0][0], results[1][0])
    np.testing.assert_array_equal(results[0][1], results[1][1])
    return results[0]


def _render(store, tab, images, field, z0, shape, mode, shared):
    """unetk_slice_prior_render into a guarded [N, D, H, W, 2] -> numpy; every element written, nothing outside."""
    from boxsegliver_amd import _abi, ops
    n = tab.shape[0]
    desc = _desc(store, n, shape, 1)
    out = guardbuf.guarded((n,) + tuple(shape) + (2,))
    code = _abi.lib().unetk_slice_prior_render(ctypes.byref(desc), _abi.ptr(tab), _abi.ptr(images), _abi.ptr(field), _abi.ptr(z0),
                                               1 if shared else 0, ops.SLICE_PRIOR_MODES[mode], ctypes.c_void_p(out.ptr()),
                                               _abi.stream_ptr())
    assert code == 0, code
    torch.cuda.synchronize()
    assert out.check_untouched() and out.unwritten() == 0
    return out.view.clone()


def _clicks(z0s, cnts, yx=(1, 2)):
    """pts int32 [N, 2, 4, 3] / cnt int32 [N, 2] whose first foreground click lies on slice z0s[n]; the other entries hold
    values that must not matter."""
    n = len(z0s)
    pts = np.full((n, 2, 4, 3), -1, np.int32)
    pts[:, 0, 0] = [(z, yx[0], yx[1]) for z in z0s]
    pts[:, 0, 1] = (0, 5, 5)                                                     # a second foreground click on another slice
    pts[:, 1, 0] = (2, 3, 3)
    cnt = np.stack([np.asarray(cnts, np.int32), np.ones(n, np.int32)], axis=1)
    return torch.from_numpy(pts).cuda(), torch.from_numpy(np.ascontiguousarray(cnt)).cuda()


# (name, case, centre, crop (ch, cw), z0, cnt, obj_label)
FIELD_CASES = [
    ("box 1 x 1 on the object", 0, (1, 17, 30), (1, 1), 0, 1, 2),
    ("box 1 x 7", 0, (1, 17, 21), (1, 7), 0, 1, 2),
    ("box 7 x 1", 0, (1, 12, 30), (7, 1), 0, 1, 2),
    ("box 37 x 70: wave tails", 0, (1, 20, 40), (37, 70), 0, 1, 1),
    ("box 37 x 70, tumour", 0, (1, 18, 36), (37, 70), 0, 1, 2),
    ("a single-pixel object", 0, (1, 20, 40), (30, 50), 1, 1, 2),
    ("a single pixel in the box's corner", 0, (1, 30, 60), (20, 39), 1, 1, 2),
    ("touching all four borders", 0, (1, 20, 40), (21, 33), 3, 1, 2),
    ("filling the box: sentinel", 0, (1, 20, 40), (25, 40), 2, 1, 1),
    ("no object on z0", 0, (1, 20, 40), (25, 40), 2, 1, 2),
    ("cnt == 0", 0, (1, 20, 40), (37, 70), 0, 0, 1),
    ("z0 on the first patch slice", 0, (6, 20, 44), (30, 64), 0, 1, 2),
    ("z0 on the last patch slice", 0, (6, 20, 44), (30, 65), 3, 1, 1),
    ("random pixels", 0, (3, 20, 40), (40, 80), 3, 1, 2),
    ("a shallow case, a real slice", 1, (1, 14, 40), (33, 66), 1, 1, 2),
    ("a shallow case, its zero-padded slice", 1, (1, 14, 40), (33, 66), 3, 1, 1),
    ("z0 beyond the patch", 0, (1, 20, 40), (20, 20), 4, 1, 1),
    ("z0 negative with a count", 0, (1, 20, 40), (20, 20), -1, 1, 1),
]


def _expected_mask(store, case, obj, box, z0, cnt, whole, depth_out):
    lab = store.cases[case]
    if whole:
        if cnt <= 0 or not 0 <= z0 < lab.shape[0]:
            return np.zeros(store.src, np.uint8)
        return (lab[z0] >= obj).astype(np.uint8)
    if cnt <= 0:
        return np.zeros(box[3:], np.uint8)
    return sref.box_mask(lab, box, z0, obj, depth_out)


@pytest.mark.parametrize("mode", ["boundary", "binary"])
@pytest.mark.parametrize("obj", [1, 2])
def test_field_equals_the_restatement_exactly(store_a, mode, obj):
    cases = [c for c in FIELD_CASES if c[6] == obj]
    shape = (D, 16, 20)
    tab = torch.from_numpy(np.stack([store_a.row(ci, c, crop) for _, ci, c, crop, _, _, _ in cases])).cuda()
    pts, cnt = _clicks([c[4] for c in cases], [c[5] for c in cases])
    boxes = [ref.crop_box(c, crop, shape, store_a.cases[ci].shape[0], store_a.src) for _, ci, c, crop, _, _, _ in cases]
    got, z0 = _field(store_a, tab, pts, cnt, shape, obj, mode, False, [b[3:] for b in boxes])
    seen = dict(sentinel=0, real=0)
    for j, ((name, ci, _, _, z, k, _), box) in enumerate(zip(cases, boxes)):
        assert z0[j] == (z if k > 0 else -1), name
        mask = _expected_mask(store_a, ci, obj, box, z, k, False, D)
        want = sref.field(mask, mode)
        np.testing.assert_array_equal(got[j, :box[3] * box[4]].reshape(box[3], box[4]), want, err_msg=name)
        seen["sentinel" if (want == sref.SENTINEL).all() else "real"] += 1
    assert seen["real"] > 0 and (mode == "binary" or seen["sentinel"] > 0), seen


def test_field_inputs_are_what_their_names_say(store_a):
    """The masks of FIELD_CASES hold the corner cases they are named after."""
    shape = (D, 16, 20)
    by = {c[0]: c for c in FIELD_CASES}

    def mask(name):
        _, ci, c, crop, z, k, obj = by[name]
        box = ref.crop_box(c, crop, shape, store_a.cases[ci].shape[0], store_a.src)
        return _expected_mask(store_a, ci, obj, box, z, k, False, D)
    assert mask("box 1 x 1 on the object").tolist() == [[1]]
    assert mask("a single-pixel object").sum() == 1 and mask("a single pixel in the box's corner")[0, 0] == 1
    m = mask("touching all four borders")
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and not m.all()
    assert mask("filling the box: sentinel").all() and not mask("no object on z0").any()
    assert mask("a shallow case, a real slice").any() and not mask("a shallow case, its zero-padded slice").any()
    assert mask("z0 on the first patch slice").any() and mask("z0 on the last patch slice").any()
    assert 0 < mask("box 1 x 7").sum() < 7 or mask("box 1 x 7").all()
    for name in ("box 37 x 70: wave tails", "box 37 x 70, tumour", "random pixels"):
        b = sref.inner_boundary(mask(name))
        assert b.any() and (b != mask(name).astype(bool)).any()                  # boundary and interior pixels both


def test_field_one_past_the_staging_length_and_the_row_block(store_b):
    """129 rows: the second staged chunk holds one row; 257 columns: the second trip of the row kernel holds one pixel."""
    shape = (2, 16, 16)
    rows = [((0, 64, 128), (STAGE + 1, 257), 0), ((0, 0, 0), (STAGE + 1, 64), 0), ((0, 129, 259), (STAGE, 257), 0),
            ((0, 65, 130), (130, 260), 1), ((0, 65, 130), (STAGE + 1, 65), 1)]
    tab = torch.from_numpy(np.stack([store_b.row(0, c, crop) for c, crop, _ in rows])).cuda()
    pts, cnt = _clicks([z for _, _, z in rows], [1] * len(rows))
    boxes = [ref.crop_box(c, crop, shape, 2, store_b.src) for c, crop, _ in rows]
    assert boxes[0][3:] == (STAGE + 1, 257) and boxes[2][1:3] == (2, 3)
    got, _ = _field(store_b, tab, pts, cnt, shape, 1, "boundary", False, [b[3:] for b in boxes])
    for j, ((_, _, z), box) in enumerate(zip(rows, boxes)):
        mask = sref.box_mask(store_b.cases[0], box, z, 1, 2)
        want = sref.field(mask)
        assert (want >= 0).all() and want.max() > 0
        np.testing.assert_array_equal(got[j, :box[3] * box[4]].reshape(box[3:]), want, err_msg=str(rows[j]))
    # the far pixel matters: its row and column are the last staged row and the lone pixel of the second row block
    assert got[2, :STAGE * 257].reshape(STAGE, 257)[-1, -1] == 0


@pytest.mark.parametrize("mode", ["boundary", "binary"])
def test_field_over_the_whole_slice(store_a, mode):
    """whole: the box is the slice, whatever the row's crop box is, and z0 counts from the case's first slice -- per row lists
    and one shared pair of lists."""
    shape = (D, 16, 20)
    rows = [(0, (9, 30, 60), (18, 22), 5, 1), (0, (0, 0, 0), (18, 22), 11, 1), (1, (1, 10, 10), (18, 22), 1, 1),
            (1, (1, 10, 10), (18, 22), 3, 1), (0, (9, 30, 60), (18, 22), 0, 0), (0, (2, 3, 4), (5, 6), 12, 1)]
    tab = torch.from_numpy(np.stack([store_a.row(ci, c, crop) for ci, c, crop, _, _ in rows])).cuda()
    pts, cnt = _clicks([r[3] for r in rows], [r[4] for r in rows])
    got, z0 = _field(store_a, tab, pts, cnt, shape, 2, mode, True, [store_a.src] * len(rows))
    for j, (ci, c, crop, z, k) in enumerate(rows):
        assert ref.crop_box(c, crop, shape, store_a.cases[ci].shape[0], store_a.src)[1:3] != (0, 0) or j in (1, 5)
        want = sref.field(_expected_mask(store_a, ci, 2, None, z, k, True, D), mode)
        np.testing.assert_array_equal(got[j].reshape(store_a.src), want, err_msg=str(rows[j]))
    assert (got[0] >= 0).all() and (got[3] <= 0).all() and (got[5] <= 0).all()   # a slice beyond the case: background
    # one pair of lists for every row: case 1's rows read ITS slice 1
    lp = torch.full((2, 5, 3), -1, dtype=torch.int32, device="cuda")
    lp[0, 0] = torch.tensor([1, 7, 7], dtype=torch.int32)
    lp[0, 1] = torch.tensor([0, 1, 1], dtype=torch.int32)
    lc = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    got, z0 = _field(store_a, tab[2:4].contiguous(), lp, lc, shape, 2, mode, True, [store_a.src] * 2)
    want = sref.field((store_a.cases[1][1] >= 2).astype(np.uint8), mode)
    assert z0.tolist() == [1, 1]
    np.testing.assert_array_equal(got[0].reshape(store_a.src), want)
    np.testing.assert_array_equal(got[1].reshape(store_a.src), want)
    got, z0 = _field(store_a, tab[2:3].contiguous(), lp, torch.zeros_like(lc), shape, 2, mode, True, [store_a.src])
    assert z0.tolist() == [-1] and (got == (sref.SENTINEL if mode == "boundary" else 0)).all()


def test_refusals_of_the_entry_points(store_a):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    tab = torch.from_numpy(np.stack([store_a.row(0, (1, 20, 40), (20, 20))])).cuda()
    pts, cnt = _clicks([0], [1])
    desc = _desc(store_a, 1, (D, 16, 20), 1)
    field = torch.empty((1, 3200), dtype=torch.int32, device="cuda")
    z0 = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(3200 * 4, dtype=torch.uint8, device="cuda")

    def call(d=desc, mode=0, k=0, nbytes=ws.numel(), wsp=ws):
        return lib.unetk_slice_prior_field(ctypes.byref(d), _abi.ptr(store_a.lb), _abi.ptr(tab), _abi.ptr(pts), _abi.ptr(cnt), k, 0,
                                           mode, _abi.ptr(field), _abi.ptr(z0), _abi.ptr(wsp), nbytes, _abi.stream_ptr())
    assert call() == 0 and call(mode=1, wsp=None, nbytes=0) == 0                  # binary needs no workspace
    assert call(mode=2) != 0 and call(k=65) != 0 and call(wsp=None) != 0 and call(nbytes=ws.numel() - 1) != 0
    big = _desc(store_a, 1, (D, 16, 20), 1)
    big.src_w = 4097
    assert lib.unetk_slice_prior_ws_bytes(ctypes.byref(big)) == 0 and call(d=big) != 0
    torch.cuda.synchronize()
    with pytest.raises(KeyError):
        ops.slice_prior_field(store_a.lb, tab, pts, cnt, (D, 16, 20), 1, "edges")


# ------------------------------------------------------------------------------------------------- render
def _flips8():
    return [(i & 1, (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]


@pytest.mark.parametrize("mode", ["boundary", "binary"])
@pytest.mark.parametrize("shape,crop,tol", [((D, 24, 36), (24, 36), IDENTITY_TOL), ((D, 16, 20), (24, 36), RESIZE_TOL),
                                            ((D, 32, 24), (21, 33), RESIZE_TOL), ((D, 16, 20), (37, 70), RESIZE_TOL)])
def test_render_matches_the_restatement(store_a, mode, shape, crop, tol):
    """All eight flip combinations on rows that hold a prior, then the sentinel rows; channel 0 is the patch bit for bit."""
    from boxsegliver_amd import ops
    flips = _flips8()
    samples = [(0, (8, 20, 40), crop, flips[i], i % D, 1) for i in range(8)]           # slices 6 .. 9 of case 0: an ellipse each
    samples += [(0, (1, 20, 40), crop, (1, 0, 1), 2, 1), (0, (1, 20, 40), crop, (0, 1, 0), 0, 0), (1, (1, 14, 40), crop, (1, 1, 1), 3, 1)]
    tab = torch.from_numpy(np.stack([store_a.row(ci, c, cr, fl) for ci, c, cr, fl, _, _ in samples])).cuda()
    pts, cnt = _clicks([s[4] for s in samples], [s[5] for s in samples])
    obj = 1
    images, _ = ops.lits_patch3d(store_a.im, store_a.lb, tab, shape, False)
    field, z0 = ops.slice_prior_field(store_a.lb, tab, pts, cnt, shape, obj, mode)
    out = _render(store_a, tab, images, field, z0, shape, mode, False)
    assert torch.equal(out[..., 0], images[..., 0])                              # bit for bit
    got = out[..., 1].cpu().numpy().astype(np.float64)
    worst, live, zero = 0.0, 0, 0
    for j, (ci, c, cr, fl, z, k) in enumerate(samples):
        box = ref.crop_box(c, cr, shape, store_a.cases[ci].shape[0], store_a.src)
        mask = _expected_mask(store_a, ci, obj, box, z, k, False, D)
        want = sref.render(sref.prior_volume(mask, z, D, mode), shape[1:], fl)
        err = float(np.abs(got[j] - want).max())
        print("slice prior render", mode, shape, crop, "row", j, "max abs dev", err)
        worst = max(worst, err)
        if not want.any():
            assert j >= 8 and not got[j].any(), j                                # sentinel rows: exactly 0
            zero += 1
        else:
            assert want.max() > 0.9, j
            live += 1
    # the row on the slice the object fills is a sentinel row under `boundary` and a slice of ones under `binary`
    assert (live, zero) == ((8, 3) if mode == "boundary" else (9, 2)) and worst <= tol, worst
    if mode == "boundary":
        assert 0.0 < got[:8].min() and got.max() <= 1.0


@pytest.mark.parametrize("mode", ["boundary", "binary"])
def test_render_of_a_shared_field(store_a, mode):
    """One whole-slice field in case coordinates for a window table of case 0 (store_a's second store case follows it, so no
    row starts at store slice 0 of another case): rows whose boxes lie before z0 (dz < 0), behind it (dz >= D) and around it,
    box origins other than 0, flips; and the per-row form fed the crops of the same field gives the same bits."""
    from boxsegliver_amd import ops
    shape, crop, z0c, obj = (D, 16, 20), (18, 22), 4, 2
    centres = [(2, 9, 11), (6, 20, 40), (10, 31, 69), (6, 9, 69), (2, 25, 45), (10, 20, 40), (7, 22, 48)]
    flips = _flips8()
    tab_np = np.stack([store_a.row(0, c, crop, flips[(i * 3) % 8]) for i, c in enumerate(centres)])
    tab = torch.from_numpy(tab_np).cuda()
    lp = torch.full((2, 6, 3), -1, dtype=torch.int32, device="cuda")
    lp[0, 0] = torch.tensor([z0c, 22, 48], dtype=torch.int32)
    lc = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    field, z0 = ops.slice_prior_field(store_a.lb, tab[:1].contiguous(), lp, lc, shape, obj, mode, whole=True)
    assert tuple(field.shape) == (1, 3200) and z0.tolist() == [z0c]
    images, _ = ops.lits_patch3d(store_a.im, store_a.lb, tab, shape, False)
    out = _render(store_a, tab, images, field, z0, shape, mode, True)
    assert torch.equal(out[..., 0], images[..., 0])
    lab = store_a.cases[0]
    vol = sref.prior_volume((lab[z0c] >= obj).astype(np.uint8), z0c, lab.shape[0], mode)
    got = out[..., 1].cpu().numpy().astype(np.float64)
    boxes = [ref.crop_box(c, crop, shape, lab.shape[0], store_a.src) for c in centres]
    dz = [(b[0] - z0c, b[0] + D - 1 - z0c) for b in boxes]
    assert any(hi < 0 for _, hi in dz) and any(lo >= D for lo, _ in dz) and any(lo <= 0 <= hi for lo, hi in dz)
    assert any(b[0] > 0 and b[1] > 0 and b[2] > 0 for b in boxes)
    worst = 0.0
    for j, (z1, y1, x1, ch, cw) in enumerate(boxes):
        want = sref.render(vol[z1:z1 + D, y1:y1 + ch, x1:x1 + cw], shape[1:], tuple(tab_np[j, 7:10]))
        worst = max(worst, float(np.abs(got[j] - want).max()))
    print("slice prior shared render", mode, "max abs dev", worst)
    assert worst <= RESIZE_TOL
    if mode == "binary":
        assert all(not got[j].any() for j, (lo, hi) in enumerate(dz) if hi < 0 or lo > 0)
    # the per-row form: each row's crop of the field, stored densely, and z0 relative to its box
    f2 = field.view(store_a.src)
    per_row = torch.zeros((len(boxes), 3200), dtype=torch.int32, device="cuda")
    for j, (z1, y1, x1, ch, cw) in enumerate(boxes):
        per_row[j, :ch * cw] = f2[y1:y1 + ch, x1:x1 + cw].reshape(-1)
    z0_rows = torch.tensor([z0c - b[0] for b in boxes], dtype=torch.int32, device="cuda")
    again = _render(store_a, tab, images, per_row, z0_rows, shape, mode, False)
    assert torch.equal(again, out)
    # no click: the channel is zero
    field0, z00 = ops.slice_prior_field(store_a.lb, tab[:1].contiguous(), lp, torch.zeros_like(lc), shape, obj, mode, whole=True)
    none = ops.slice_prior_render(tab, images, field0, z00, shape, store_a.src, mode, shared=True)
    assert not none[..., 1].any() and torch.equal(none[..., 0], images[..., 0])


# ------------------------------------------------------------------------------------------------- pipeline
def _train_argv(root, extra):
    argv = ("liver_3d --mode train --tag prior3d --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm --num_of_steps 4 "
            "--batches_per_epoch 2 --eval_num_batches_per_epoch 2 --evaluator Volume --loss_weight_type numerical "
            "--loss_numeric_w 0.2 0.4 4.4 --learning_rate 0.001 --log_step 1 --use_spatial --local_enhance").split()
    return argv + extra.split() + ["--lits_root", str(root), "--model_dir", str(root / "run")]


@pytest.mark.parametrize("mode", ["boundary", "binary"])
def test_batches_with_a_prior_and_one_training_step(tmp_path, mode):
    from boxsegliver_amd.NetworksV2.UNet3D import UNet3D
    from boxsegliver_amd.core.solver import Solver
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    import test_gpu_unet3d as t3
    ref.write_dataset(tmp_path)
    args, _, _ = entry.get_arguments(_train_argv(tmp_path, "--im_channel 2 --slice_prior " + mode))
    plain_args, _, _ = entry.get_arguments(_train_argv(tmp_path, "--im_channel 1"))
    batches = {}
    for name, a in (("prior", args), ("plain", plain_args)):
        for split in ("train", "eval_online"):
            gen = lits3d.input_fn(split, {"args": a, "lits_root": str(tmp_path)})
            batches[name, split] = [next(gen) for _ in range(2 if split == "eval_online" else 3)]
    hits = 0
    for split in ("train", "eval_online"):
        for (fa, la), (fb, lb) in zip(batches["prior", split], batches["plain", split]):
            assert fa["images"].shape == (2, 4, 32, 32, 2) and fa["images"].dtype == torch.float32 and fb["images"].shape[-1] == 1
            # the same seeds without the flag: labels, guide and image bit for bit -- the prior draws nothing
            assert torch.equal(la, lb) and torch.equal(fa["sp_guide"], fb["sp_guide"])
            assert torch.equal(fa["images"][..., 0], fb["images"][..., 0])
            prior = fa["images"][..., 1]
            assert bool(torch.isfinite(prior).all()) and 0.0 <= float(prior.min()) and float(prior.max()) <= 1.0
            hits += int(float(prior.max()) > 0.5)                                 # the forced sample holds its object: a click
    assert hits >= 3
    feats, labels = batches["prior", "train"][0]
    margs = t3.make_args(classes=["Liver", "Tumor"], im_channel=2, use_spatial=True, guide_channel=2, loss_numeric_w=[0.2, 0.4, 4.4])
    model = UNet3D(margs)
    inputs = dict(feats, labels=labels)
    model(inputs, "eval", **t3.YML)
    before = {k: v.clone() for k, v in model.params.state_dict().items()}
    assert before["UNet3D/conv_e0/conv1/weights"].shape == (1, 3, 3, 4, 30)       # image, prior and the two guide channels
    solver = Solver(margs)
    loss = model(inputs, "train", **t3.YML)
    assert np.isfinite(loss.item())
    solver(loss, model)
    after = model.params.state_dict()
    first = "UNet3D/conv_e0/conv1/weights"
    assert not torch.equal(after[first][..., 1, :], before[first][..., 1, :])     # the prior channel's filters moved
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    with pytest.raises(ValueError, match="images must be"):
        model(dict(inputs, images=feats["images"][..., :1].contiguous()), "eval", **t3.YML)


def test_main_eval_3d_with_a_prior(tmp_path, monkeypatch):
    """The field is built once per session from the first click and every later round renders that very field; the run
    without the flag gives the trace it gives without this feature's hook (prior=None is the old call)."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.entry import main_eval_3d
    import test_gpu_inter_eval3d as ti
    cases = ref.write_dataset(tmp_path)
    extra = "--use_spatial --local_enhance --max_iter 3".split()
    built, rendered = [], []
    real_field, real_render = ops.slice_prior_field, ops.slice_prior_render

    def field_spy(*a, **kw):
        out = real_field(*a, **kw)
        built.append((out[0].clone(), out[1].clone(), out[0], kw.get("whole")))
        return out

    def render_spy(tab, images, field, z0, *a, **kw):
        rendered.append((field, int(z0.item()), bool(kw.get("shared")), torch.equal(field, built[-1][0])))
        return real_render(tab, images, field, z0, *a, **kw)
    monkeypatch.setattr(ops, "slice_prior_field", field_spy)
    monkeypatch.setattr(ops, "slice_prior_render", render_spy)
    argv = ti._eval_argv(tmp_path, "Tumor", extra + ["--slice_prior", "boundary"])
    argv[argv.index("--im_channel") + 1] = "2"
    trace, volumes = [], {}
    results = main_eval_3d.run(main_eval_3d.get_arguments(argv), trace=trace, restore=False, volumes=volumes)
    assert sorted(volumes) == [2, 3] and 0.0 <= results["G_Dice"] <= 1.0
    assert len(built) == 2                                                       # once per session
    forwards = {pid: sum(1 for r in trace if r[0] == pid and r[5] is None) for pid in (2, 3)}
    assert max(forwards.values()) >= 2                                           # a session with rounds after the first click
    assert len(rendered) >= sum(forwards.values()) and all(r[2] and r[3] for r in rendered)
    for (snap, z0, live, whole), pid in zip(built, (2, 3)):
        assert whole is True and torch.equal(snap, live)                         # unchanged by the later clicks and rounds
        first = [r for r in trace if r[0] == pid][0]
        assert first[2] == 0 and int(z0.item()) == first[1][0]                   # round 0 places a foreground click: its slice
        want = sref.field((cases[pid][1][first[1][0]] >= 2).astype(np.uint8))
        np.testing.assert_array_equal(snap.cpu().numpy().reshape(ref.H, ref.W), want)
    # without the flag: no field, no render, and the trace of the run as it was
    del built[:], rendered[:]
    plain = ti._eval_argv(tmp_path, "Tumor", extra)
    t1, t2 = [], []
    main_eval_3d.run(main_eval_3d.get_arguments(plain), trace=t1, restore=False)
    assert not built and not rendered
    monkeypatch.undo()
    main_eval_3d.run(main_eval_3d.get_arguments(plain), trace=t2, restore=False)
    assert t1 == t2 and len(t1) >= 2
