"""No GPU: the library's host queries agree with the tables of tests/test_gpu_conv_epilogue_paths.py.

unetk_conv3x3_fwd_affine_ok, unetk_conv3x3_stat_rows, unetk_conv3x3_dgrad_nbr_rows and unetk_conv3x3_ws_bytes all read the plan
the launch reads (csrc/conv_igemm.hip, unetk_conv_plan) and are pure host arithmetic: for every row of the two tables the stated
admission (with and without the pool), the stated row counts, the refusals, and the stream-K scratch exactly where a row names
the stream-K kernels.  The affine rows are asked with the padded output stride the GPU test uses (Cout + 64).
"""
import ctypes

import pytest

from test_gpu_conv_epilogue_paths import (AFF_ROWS, AFF_ODD_POOL, NBR_ROWS, NBR_REFUSED, NBR_MISALIGNED, NBR_BY_ID, FP32, BF16,
                                          E_BADARG)


@pytest.fixture(scope="module")
def L():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    lib.unetk_conv3x3_ws_bytes.restype = ctypes.c_size_t
    return lib


def _desc(n, h, w, cin, cout, prec, ys=None):
    from boxsegliver_amd import _abi
    return _abi.ConvDesc(n, h, w, cin, cout, cin, ys or cout, prec, 1)


@pytest.mark.parametrize("row", AFF_ROWS, ids=[r.id for r in AFF_ROWS])
def test_affine_rows(L, row):
    for ys in (row.cout, row.cout + 64):
        d = _desc(row.n, row.h, row.w, row.cin, row.cout, row.prec, ys)
        assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 0) == int(row.ok)
        assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 1) == int(row.ok and row.pool)
        assert L.unetk_conv3x3_stat_rows(ctypes.byref(d)) == row.rows
        # no affine row has a fused reduction: fewer than 128 channels on one side, or a plane of the linear-pixel kernel
        assert L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(d)) == 0
        sk = row.kern is not None and any("lin_sk_fixup_kernel" in k for k in row.kern)
        if row.prec == FP32:
            assert (L.unetk_conv3x3_ws_bytes(ctypes.byref(d)) > 0) == sk
        else:
            assert L.unetk_conv3x3_ws_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("shape", AFF_ODD_POOL, ids=["%dx%d" % (s[1], s[2]) for s in AFF_ODD_POOL])
def test_pool_on_odd_extents_is_refused(L, shape):
    d = _desc(*shape)
    assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 0) == 1
    assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 1) == 0


@pytest.mark.parametrize("row", NBR_ROWS, ids=[r.id for r in NBR_ROWS])
def test_nbr_rows(L, row):
    d = _desc(row.n, row.h, row.w, row.cin, row.cout, row.prec)
    assert L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(d)) == row.rows
    assert row.rows % row.n == 0
    assert L.unetk_conv3x3_stat_rows(ctypes.byref(d)) == row.frows
    assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 1) == int(row.prec == FP32)      # bf16 storage: 156 / 18 forward tiles, no persistent kernel
    assert L.unetk_conv3x3_ws_bytes(ctypes.byref(d)) == 0
    # the same shape in UNETK_BF16 has no fused variant
    assert L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(_desc(row.n, row.h, row.w, row.cin, row.cout, BF16))) == 0


@pytest.mark.parametrize("what,shape,prec", NBR_REFUSED, ids=[r[0] for r in NBR_REFUSED])
def test_nbr_refusals(L, what, shape, prec):
    assert L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(_desc(*(shape + (prec,))))) == 0


@pytest.mark.parametrize("what,rid,off,extra", NBR_MISALIGNED, ids=[m[0] for m in NBR_MISALIGNED])
def test_nbr_misaligned_prod_y_is_refused_on_the_host(L, what, rid, off, extra):
    """The alignment rule of include/unetk.h is checked before anything touches the device: with fabricated (never
    dereferenced) addresses the entry point returns UNETK_E_BADARG on a machine without a GPU."""
    r = NBR_BY_ID[rid]
    d = _desc(r.n, r.h, r.w, r.cin, r.cout, r.prec)
    base = 1 << 20
    P = ctypes.c_void_p
    rc = L.unetk_conv3x3_dgrad_nbr(ctypes.byref(d), P(base), P(base), P(base), P(base + off), r.cin + extra, P(base), P(base),
                                   P(base), P(base), 0, P(base), None)
    assert rc == E_BADARG, (what, rc)
