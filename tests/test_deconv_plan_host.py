"""No GPU: the transposed conv's workspace queries are the plan of the launch (csrc/deconv.hip deconv_plan).

The backward (unetk_deconv3d_bwd_parts) and the queries read one plan, and the queries are pure host arithmetic, so they can be
asked without a device.  A query is a function of exactly the splits S of the filter gradient and the blocks of
relu_bwd_bias_kernel (test_gpu_deconv_paths.ws_bytes_of), for the precision the descriptor names; a refused backward asks for 0,
and is refused before the plan divides by anything the shape could make zero.
"""
import ctypes

import pytest

from test_gpu_deconv_paths import ROWS, BY_ID, PLANS, REFUSALS, FP32, BF16, BF16S, PREC_NAME, bwd_ok, plan, ws_bytes_of

PRECS = (FP32, BF16, BF16S)


@pytest.fixture(scope="module")
def L():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_deconv3d_bwd_ws_bytes", "unetk_deconv2x2_bwd_ws_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
    return lib


def _q3(L, n, d, h, w, cin, cout, kd, stride, coff, prec):
    from boxsegliver_amd import _abi
    return L.unetk_deconv3d_bwd_ws_bytes(ctypes.byref(_abi.Deconv3dDesc(n, d, h, w, cin, cout, kd, stride, coff, prec)))


def _q2(L, n, h, w, cin, cout, stride, coff, prec):
    from boxsegliver_amd import _abi
    return L.unetk_deconv2x2_bwd_ws_bytes(ctypes.byref(_abi.DeconvDesc(n, h, w, cin, cout, stride, coff, prec)))


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_query_is_the_restated_plan_in_every_precision(L, row):
    """Every row, all three precisions (those the row does not list included): the restated plan's bytes where the restated
    backward rules admit the shape, 0 where they refuse it; a 2-D row asks the same through the 2-D query."""
    for prec in PRECS:
        want = 0
        if bwd_ok(row, prec):
            S, _, nblk = plan(row, prec)
            want = ws_bytes_of(row, S, nblk)
            assert want > 0
        got = _q3(L, row.n, row.d, row.h, row.w, row.cin, row.cout, row.kd, row.stride, row.coff, prec)
        assert got == want, (PREC_NAME[prec], got, want)
        if row.api == "2d":
            got = _q2(L, row.n, row.h, row.w, row.cin, row.cout, row.stride, row.coff, prec)
            assert got == want, (PREC_NAME[prec], "2d", got, want)


@pytest.mark.parametrize("rid,prec", sorted(PLANS), ids=["{}-{}".format(r, PREC_NAME[q]) for r, q in sorted(PLANS)])
def test_query_is_exact_for_the_plans_of_the_table(L, rid, prec):
    r = BY_ID[rid]
    S, _, nblk = PLANS[(rid, prec)]
    assert _q3(L, r.n, r.d, r.h, r.w, r.cin, r.cout, r.kd, r.stride, r.coff, prec) == ws_bytes_of(r, S, nblk)


BWD_REFUSALS = [r for r in REFUSALS if r[1] == "bwd"]


@pytest.mark.parametrize("what,call,shape,code", BWD_REFUSALS, ids=[r[0] for r in BWD_REFUSALS])
def test_refused_backward_asks_for_nothing(L, what, call, shape, code):
    """The shapes of test_gpu_deconv_paths.test_refusals, through the row's own API."""
    api, cin, cout, kd, stride, coff, prec = shape
    n, dd, h, w = 1, (2 if api == "3d" else 1), 2, 3
    if api == "2d":
        assert _q2(L, n, h, w, cin, cout, stride, coff, prec) == 0
    else:
        assert _q3(L, n, dd, h, w, cin, cout, kd, stride, coff, prec) == 0


@pytest.mark.parametrize("cout", [1028, 2048, 4096])
def test_more_than_1024_channels_are_refused_before_the_plan_divides(L, cout):
    """Cout > 1024 leaves relu_bwd_bias_kernel's thread map (unetk_colmap) zero rows per block: a planner that divided by it
    before refusing would end the process here."""
    for prec in PRECS:
        assert _q2(L, 1, 2, 3, 64, cout, 2 * cout, cout, prec) == 0, PREC_NAME[prec]
        assert _q3(L, 1, 2, 2, 3, 64, cout, 2, 2 * cout, cout, prec) == 0, PREC_NAME[prec]
