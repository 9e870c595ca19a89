"""The volume-evaluation entry points of the C ABI without a GPU (include/unetk.h, csrc/evalvol.hip): the workspace
queries, and the refusals that return before anything is launched -- NULL pointers, bad extents, more than 2^31 voxels."""
import ctypes

from boxsegliver_amd import _abi

E_BADARG, E_UNSUPPORTED = -1, -2
NAMES = ("unetk_largest_component_ws_bytes", "unetk_largest_component", "unetk_component_mask", "unetk_mask_counts_ws_bytes", "unetk_mask_counts",
         "unetk_surface3d", "unetk_edt3d_sq_ws_bytes", "unetk_edt3d_sq", "unetk_surface_dist_ws_bytes", "unetk_surface_dist")


def test_entry_points_are_exported_and_bound():
    lib = _abi.lib()
    for name in NAMES:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.unetk_abi_version() == _abi.ABI_VERSION == 10


def test_workspace_queries():
    lib = _abi.lib()
    d, h, w = 7, 13, 17
    n = d * h * w
    assert lib.unetk_largest_component_ws_bytes(d, h, w) >= 8 * n + 8
    assert lib.unetk_edt3d_sq_ws_bytes(d, h, w) >= 20 * n
    assert lib.unetk_mask_counts_ws_bytes(d, h, w) >= 32
    assert lib.unetk_surface_dist_ws_bytes(d, h, w) >= 32
    assert lib.unetk_mask_counts_ws_bytes(450, 512, 512) == lib.unetk_surface_dist_ws_bytes(450, 512, 512) == 1024 * 32
    for dims in ((0, 4, 4), (4, -1, 4), (2048, 1024, 1024), (1 << 16, 1 << 15, 1)):
        for q in ("largest_component", "mask_counts", "edt3d_sq", "surface_dist"):
            assert getattr(lib, "unetk_{}_ws_bytes".format(q))(*dims) == 0, (q, dims)
    assert lib.unetk_largest_component_ws_bytes(1291, 1291, 1291) == 0          # 2^31 + a little
    assert lib.unetk_largest_component_ws_bytes(1, 1, (1 << 31) - 1) > 0


def test_refusals_return_before_any_launch():
    lib = _abi.lib()
    d, h, w = 7, 13, 17
    c = ctypes.c_double(1.0)
    assert lib.unetk_largest_component(None, d, h, w, None, None, None, 1 << 20, None) == E_BADARG
    assert lib.unetk_component_mask(None, d, h, w, 0, None, None) == E_BADARG
    assert lib.unetk_mask_counts(None, None, d, h, w, None, None, 1 << 20, None) == E_BADARG
    assert lib.unetk_surface3d(None, d, h, w, None, None, 0, None) == E_BADARG
    assert lib.unetk_edt3d_sq(None, d, h, w, None, c, c, c, None, None, 1 << 20, None) == E_BADARG
    assert lib.unetk_surface_dist(None, None, d, h, w, None, None, 1 << 20, None) == E_BADARG
    assert lib.unetk_largest_component(None, 0, h, w, None, None, None, 0, None) == E_BADARG
    D, H, W = 2048, 1024, 1024
    assert lib.unetk_largest_component(None, D, H, W, None, None, None, 0, None) == E_UNSUPPORTED
    assert lib.unetk_component_mask(None, D, H, W, 0, None, None) == E_UNSUPPORTED
    assert lib.unetk_mask_counts(None, None, D, H, W, None, None, 0, None) == E_UNSUPPORTED
    assert lib.unetk_surface3d(None, D, H, W, None, None, 0, None) == E_UNSUPPORTED
    assert lib.unetk_edt3d_sq(None, D, H, W, None, c, c, c, None, None, 0, None) == E_UNSUPPORTED
    assert lib.unetk_surface_dist(None, None, D, H, W, None, None, 0, None) == E_UNSUPPORTED
