"""Host side of the device-resident volume evaluation (CPU): the index tables of the zoom back (ops.zoom_tables) against
scipy.ndimage.zoom itself, the bilinear taps factored out of cv2_resize_linear, and the two new C entry points
(csrc/evalio.hip) in the header, the binding table and the library."""
import ctypes
import os
import re

import numpy as np
import scipy.ndimage as ndi

from boxsegliver_amd import _abi, ops
from boxsegliver_amd.data import lits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source, target) of the device zoom's GPU test (test_gpu_evalio.py); the first two and the last hit scipy's outside sample
ZOOM_CASES = [((5, 32, 48), (5, 16, 24)), ((3, 64, 64), (3, 93, 78)), ((4, 64, 64), (4, 92, 80)), ((1, 40, 23), (1, 37, 5)),
              ((2, 16, 16), (2, 16, 16)), ((3, 24, 40), (7, 24, 131))]


def gather_with_tables(vol, tables):
    """vol[tz][:, ty][:, :, tx] with -1 = 0: fancy indexing into the array padded with one zero plane at the END of every
    axis, which is where index -1 points."""
    padded = np.pad(vol, [(0, 1)] * vol.ndim)
    return padded[np.ix_(*tables)]


def _check(in_shape, out_shape, rng):
    vol = rng.randint(0, 3, size=in_shape).astype(np.uint8)
    ref = ndi.zoom(vol, np.array(out_shape) / np.array(in_shape), order=0)
    tables = ops.zoom_tables(in_shape, out_shape)
    assert ref.shape == tuple(out_shape)
    assert [t.shape for t in tables] == [(n,) for n in out_shape] and all(t.dtype == np.int32 for t in tables)
    assert all(t.min() >= -1 and t.max() < n for t, n in zip(tables, in_shape))
    np.testing.assert_array_equal(gather_with_tables(vol, tables), ref, err_msg="{} -> {}".format(in_shape, out_shape))
    return any((t < 0).any() for t in tables)


def test_zoom_tables_reproduce_scipy_zoom_order0():
    rng = np.random.RandomState(7)
    outside = [_check(i, o, rng) for i, o in ZOOM_CASES]
    assert sum(outside) >= 2                                   # the listed cases do exercise the outside-sample rule
    hits = 0
    for _ in range(500):
        in_shape = tuple(int(v) for v in rng.randint(1, 40, size=3))
        out_shape = tuple(int(v) for v in rng.randint(1, 60, size=3))
        hits += _check(in_shape, out_shape, rng)
    assert hits > 0                                            # ... and so do random shapes (about one in six)
    # the pairs of the report that motivated the tables: the last sample of the axis is outside
    for n_in, n_out in ((32, 16), (48, 24), (64, 78), (64, 93), (256, 368)):
        (t,) = ops.zoom_tables((n_in,), (n_out,))
        assert t[-1] == -1 and (t[:-1] >= 0).all(), (n_in, n_out)
    (t,) = ops.zoom_tables((17,), (17,))
    np.testing.assert_array_equal(t, np.arange(17))


def test_cv2_linear_taps_restate_the_resize():
    rng = np.random.RandomState(3)
    for shape, dsize in (((7, 9, 3), (5, 4)), ((10, 8, 2), (8, 10)), ((5, 5, 1), (13, 3)), ((6, 11, 4), (11, 7))):
        img = rng.rand(*shape).astype(np.float32)
        y0, y1, fy = lits.cv2_linear_taps(dsize[1], shape[0])
        x0, x1, fx = lits.cv2_linear_taps(dsize[0], shape[1])
        assert fy.dtype == np.float32 and fx.dtype == np.float32
        assert y0.min() >= 0 and y1.max() <= shape[0] - 1 and x0.min() >= 0 and x1.max() <= shape[1] - 1
        one = np.float32(1.0)
        rows = img[y0] * (one - fy)[:, None, None] + img[y1] * fy[:, None, None]
        ref = rows[:, x0] * (one - fx)[None, :, None] + rows[:, x1] * fx[None, :, None]
        got = lits.cv2_resize_linear(img, dsize)
        assert got.dtype == np.float32 and np.array_equal(got, ref)
    # equal sizes: identity taps, so the tap rule also reproduces the function's early return
    y0, y1, fy = lits.cv2_linear_taps(9, 9)
    np.testing.assert_array_equal(y0, np.arange(9))
    assert not fy.any()


def test_window_table_is_the_hosts_normalisation():
    lut = lits.window_table()
    assert lut.dtype == np.float32 and lut.shape == (lits.GRAY_MAX - lits.GRAY_MIN + 1,)
    hu = np.arange(-1100, 1400, dtype=np.int16).reshape(-1, 1, 1)
    ref = lits._window_normalise(hu).reshape(-1)
    np.testing.assert_array_equal(lut[np.clip(hu.reshape(-1), lits.GRAY_MIN, lits.GRAY_MAX) - lits.GRAY_MIN], ref)
    assert lut[0] == 0.0 and lut[-1] == 1.0 and lut[200] == np.float32(200 / 450)


def test_evalio_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "unetk.h")).read()
    lib = _abi.lib()
    for name in ("unetk_eval_slab", "unetk_zoom_nearest3d"):
        assert re.search(r"\b{}\s*\(".format(name), hdr), name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "evalio" in open(os.path.join(ROOT, "boxsegliver_amd", "csrc", "build.sh")).read()
    # argument errors are answered before anything touches a device
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.unetk_zoom_nearest3d(p, 0, 4, 4, p, p, p, 2, 2, 2, p, None) == -1
    assert lib.unetk_zoom_nearest3d(p, 2, 2, 2, p, p, p, 1 << 11, 1 << 10, 1 << 10, p, None) == -1
    assert lib.unetk_eval_slab(p, 2, 4, 4, p, 1, 1, p, p, p, 0, p, p, p, 4, p, 451, -200, 250, p, None) == -1
    assert lib.unetk_eval_slab(p, 2, 4, 4, p, 1, 1, p, p, p, 4, p, p, p, 4, p, 450, -200, 250, p, None) == -1     # short lut
    assert lib.unetk_eval_slab(p, 2, 4, 4, p, 1 << 10, 4, p, p, p, 1 << 10, p, p, p, 1 << 9, p, 451, -200, 250, p, None) == -1


def test_guided_entry_point_keeps_host_volumes(tmp_path, monkeypatch):
    """main_g hands each case's volume to the scoring step as a host array (tests/test_gpu_propagation.py reads it there),
    so only the unguided entry point asks for volumes_on="device"."""
    from boxsegliver_amd.entry import main as entry
    asked = []

    class Stop(Exception):
        pass

    def fake(*a, **k):
        asked.append(k.get("volumes_on", "host"))
        raise Stop

    for guided in (False, True):
        argv = ("liver --mode eval --tag t --model {} --classes Liver Tumor --test_fold 2 --im_height 32 --im_width 32 "
                "--evaluator Volume").format("GUNet --model_config GUNet_SP.yml" if guided else "UNet")
        args, sub, pipe = entry.get_arguments(argv.split() + ["--model_dir", str(tmp_path)], guided=guided)
        monkeypatch.setattr(pipe[3], "get_evaluator", fake)
        try:
            entry.run(args, sub, pipe, guided=guided)
        except Stop:
            pass
    assert asked == ["device", "host"]
