"""GPU: the two kernels of csrc/evalio.hip against the host code they replace -- ops.zoom_nearest3d against
scipy.ndimage.zoom(order=0) voxel for voxel (including scipy's zero samples just outside the input), ops.eval_slab against
the host pipeline (np.pad, _window_normalise, cv2_resize_linear, the channel window) bit for bit -- with every output inside
a sentinel-filled allocation and every input inside a poisoned one."""
import ctypes

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu


def _inside(data, fill, offset=0):
    """`data` as a dense view in the middle of a larger flat device allocation filled with `fill`; the view starts
    `offset` elements past a 256-byte boundary.  Returns (view, flat, snapshot of flat, mask of the view)."""
    data = torch.as_tensor(data)
    guard = max(4096, (data.numel() + 127) // 128 * 128) + offset
    flat = torch.full((2 * guard + data.numel(),), fill, dtype=data.dtype, device="cuda")
    view = flat[guard:guard + data.numel()].view(data.shape)
    view.copy_(data)
    mask = torch.zeros(flat.numel(), dtype=torch.bool, device="cuda")
    mask[guard:guard + data.numel()] = True
    return view, flat, flat.clone(), mask


# ------------------------------------------------------------------------------------------------- zoom back
@pytest.fixture(scope="module")
def zoom_refs():
    """(source volume, scipy's zoom of it, the host tables) per size pair, computed once."""
    from test_evalio_host import ZOOM_CASES
    from boxsegliver_amd import ops
    rng = np.random.RandomState(11)
    refs = []
    for in_shape, out_shape in ZOOM_CASES:
        vol = rng.randint(0, 3, size=in_shape).astype(np.uint8)
        refs.append((vol, ndi.zoom(vol, np.array(out_shape) / np.array(in_shape), order=0),
                     ops.zoom_tables(in_shape, out_shape)))
    return refs


def test_zoom_cases_contain_outside_samples(zoom_refs):
    assert sum(any((t < 0).any() for t in tables) for _, _, tables in zoom_refs) >= 2


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("offset", [0, 1])
def test_zoom_nearest3d_equals_scipy_inside_guard_bands(zoom_refs, case, offset):
    """offset 0: 16-byte stores with a byte tail; offset 1: the output is not 16-byte aligned (byte stores)."""
    from boxsegliver_amd import ops
    vol, ref, tables = zoom_refs[case]
    src, src_flat, src_snap, _ = _inside(vol, 0xA5)
    out, flat, snap, mask = _inside(np.full(ref.shape, 0xA5, np.uint8), 0xA5, offset)
    assert out.data_ptr() % 16 == offset
    got = ops.zoom_nearest3d(src, ref.shape, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), torch.from_numpy(ref))
    assert torch.equal(flat[~mask], snap[~mask])               # nothing written outside the view
    assert int((flat[mask] == 0xA5).sum()) == 0                # every voxel of the view written
    assert torch.equal(src_flat, src_snap)
    # the same through explicit tables and a fresh output
    assert torch.equal(ops.zoom_nearest3d(src, ref.shape, tables=tables).cpu(), torch.from_numpy(ref))


def test_zoom_nearest3d_rejects_bad_tables_and_extents():
    from boxsegliver_amd import _abi, ops
    src = torch.zeros((2, 4, 4), dtype=torch.uint8, device="cuda")
    good = ops.zoom_tables((2, 4, 4), (2, 6, 6))
    for axis, bad in ((1, 4), (2, -2), (0, 2)):
        tables = [t.copy() for t in good]
        tables[axis][0] = bad
        with pytest.raises(ValueError):
            ops.zoom_nearest3d(src, (2, 6, 6), tables=tables)
    out, flat, snap, _ = _inside(np.full((2, 6, 6), 0xA5, np.uint8), 0xA5)
    tabs = torch.zeros(16, dtype=torch.int32, device="cuda")
    lib, p = _abi.lib(), _abi.ptr
    for d, hh in ((0, 6), (2, 0)):
        assert lib.unetk_zoom_nearest3d(p(src), d, 4, 4, p(tabs), p(tabs), p(tabs), 2, hh, 6, p(out), _abi.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(flat, snap)                             # nothing was launched


# ------------------------------------------------------------------------------------------------- slab building
def _host_slabs(vol, c, n, out_hw):
    """The host pipeline on a whole volume served as n-sample slabs of c channels: context beyond the volume is padded with
    HU 0 BEFORE the window (parse_case_eval), the slices that complete the last slab with zeros AFTER it
    (get_dataset_for_eval_image_v2).  Returns (planes for zsrc, [slab f32 [n, H, W, c]])."""
    from boxsegliver_amd.data import lits
    d, h, w = vol.shape
    lhc = (c - 1) // 2
    rhc = c - 1 - lhc
    pads = -d % n
    v = lits._window_normalise(np.pad(vol, ((lhc, rhc), (0, 0), (0, 0))))
    v = np.pad(v, ((0, 0), (0, 0), (0, pads)))
    if tuple(out_hw) != (h, w):
        v = lits.cv2_resize_linear(v, (out_hw[1], out_hw[0]))
    win = np.lib.stride_tricks.sliding_window_view(v, c, axis=-1)
    slabs = [np.ascontiguousarray(np.moveaxis(win[:, :, i:i + n], 2, 0)) for i in range(0, d + pads, n)]
    planes = [-2] * lhc + list(range(d)) + [-2] * rhc + [-1] * pads
    return np.asarray(planes, np.int32), slabs


SLAB_CASES = [((7, 48, 40), (64, 64), 4, 3),      # -2 context at both ends, -1 planes in the last slab
              ((7, 48, 40), (32, 24), 4, 1),      # downscale, not square
              ((5, 37, 53), (37, 53), 5, 2),      # no resize; 19610 elements: two past the last 16-byte store
              ((9, 80, 72), (96, 112), 2, 5)]     # more pixels than one block


@pytest.fixture(scope="module")
def slab_refs():
    rng = np.random.RandomState(23)
    refs = []
    for shape, out_hw, n, c in SLAB_CASES:
        vol = rng.randint(-1200, 1501, size=shape).astype(np.int16)          # both clamps of the window act
        refs.append((vol,) + _host_slabs(vol, c, n, out_hw))
    return refs


def _tables(vol, out_hw):
    from boxsegliver_amd.data import lits
    return lits.cv2_linear_taps(out_hw[0], vol.shape[1]), lits.cv2_linear_taps(out_hw[1], vol.shape[2]), lits.window_table()


@pytest.mark.parametrize("case", range(4))
def test_eval_slab_equals_host_pipeline_inside_guard_bands(slab_refs, case):
    from guardbuf import guarded
    from boxsegliver_amd import ops
    _, out_hw, n, c = SLAB_CASES[case]
    vol, planes, slabs = slab_refs[case]
    assert (planes == -1).any() or case == 2
    assert (planes == -2).any() or c == 1
    taps_y, taps_x, lut = _tables(vol, out_hw)
    # inputs in poisoned allocations: HU 32767 around the volume, wild indices around the tables, a huge value around lut
    vol_d, vol_flat, vol_snap, _ = _inside(vol, 32767)
    ints = [_inside(np.asarray(t, np.int32), 1 << 20)[0] for t in (taps_y[0], taps_y[1], taps_x[0], taps_x[1])]
    floats = [_inside(np.asarray(t, np.float32), 1e30)[0] for t in (taps_y[2], taps_x[2], lut)]
    zsrc_all = np.lib.stride_tricks.sliding_window_view(planes, c)
    for k, ref in enumerate(slabs):
        zsrc = _inside(np.ascontiguousarray(zsrc_all[k * n:(k + 1) * n]), 1 << 20)[0]
        g = guarded((n,) + tuple(out_hw) + (c,))
        got = ops.eval_slab(vol_d, zsrc, (ints[0], ints[1], floats[0]), (ints[2], ints[3], floats[1]), floats[2], out_hw, c,
                            out=g.view)
        assert got.data_ptr() == g.view.data_ptr()
        assert torch.equal(g.view.cpu(), torch.from_numpy(ref)), (case, k)
        assert g.check_untouched() and g.unwritten() == 0
    assert torch.equal(vol_flat, vol_snap)
    # host tables (uploaded by the wrapper) and a fresh output give the same slab
    got = ops.eval_slab(vol_d, zsrc_all[:n], taps_y, taps_x, lut, out_hw, c)
    assert torch.equal(got.cpu(), torch.from_numpy(slabs[0]))


def test_eval_slab_unaligned_output_takes_single_stores(slab_refs):
    from boxsegliver_amd import ops
    _, out_hw, n, c = SLAB_CASES[2]
    vol, planes, slabs = slab_refs[2]
    taps_y, taps_x, lut = _tables(vol, out_hw)
    sentinel = float(np.float32(-12345.0))
    out, flat, snap, mask = _inside(np.full(slabs[0].shape, sentinel, np.float32), sentinel, offset=1)
    assert out.data_ptr() % 16 == 4
    zsrc = np.lib.stride_tricks.sliding_window_view(planes, c)[:n]
    ops.eval_slab(torch.from_numpy(vol).cuda(), zsrc, taps_y, taps_x, lut, out_hw, c, out=out)
    assert torch.equal(out.cpu(), torch.from_numpy(slabs[0]))
    assert torch.equal(flat[~mask], snap[~mask])


def test_eval_slab_argument_errors_launch_nothing(slab_refs):
    from guardbuf import guarded
    from boxsegliver_amd import _abi
    vol, _, _ = slab_refs[0]
    taps_y, taps_x, lut = _tables(vol, (64, 64))
    dev = [torch.from_numpy(np.asarray(t, dt)).cuda() for t, dt in
           ((vol, np.int16), (np.zeros((4, 3)), np.int32), (taps_y[0], np.int32), (taps_y[1], np.int32), (taps_y[2], np.float32),
            (taps_x[0], np.int32), (taps_x[1], np.int32), (taps_x[2], np.float32), (lut, np.float32))]
    v, zs, y0, y1, fy, x0, x1, fx, lt = (_abi.ptr(t) for t in dev)
    g = guarded((4, 64, 64, 3))
    lib, out, st = _abi.lib(), ctypes.c_void_p(g.ptr()), _abi.stream_ptr()

    def call(d=7, n=4, c=3, h=64, w=64, lut_n=451):
        return lib.unetk_eval_slab(v, d, 48, 40, zs, n, c, y0, y1, fy, h, x0, x1, fx, w, lt, lut_n, -200, 250, out, st)

    for kw in (dict(d=0), dict(n=0), dict(c=0), dict(h=0), dict(w=-1), dict(lut_n=450), dict(n=1 << 20, h=1 << 10)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert g.changed_anywhere() == 0
    assert call() == 0                                         # the same pointers with valid extents do run
    torch.cuda.synchronize()
    assert g.unwritten() == 0 and g.check_untouched()
