"""No GPU: the filter gradient's workspace queries are the plan of the launch (csrc/conv_wgrad.hip unetk_wgrad_plan).

The launch (unetk_wgrad_run) and the queries read one plan, and the queries are pure host arithmetic, so they can be asked
without a device.  A 2-D query is exactly 256 + S x 9 Cin Cout x 4 bytes for the S of the launch the descriptor names, its
precision and dilation included; a 3-D query is the largest plan among the launches csrc/conv3d.hip wg_runs enumerates for the
layer, each planned at the plane count it runs.
"""
import ctypes

import pytest

import conv3d_bf16_cases as c3
from test_gpu_conv_paths import CASES, BY_ID, WG_PLANS, FP32, BF16, BF16S

IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def L():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_conv3x3_wgrad_ws_bytes", "unetk_conv3d_ws_bytes", "unetk_conv3d_ws_bytes_bf16"):
        getattr(lib, name).restype = ctypes.c_size_t
    return lib


def _query(L, n, h, w, cin, cout, prec, dil=1):
    from boxsegliver_amd import _abi
    return L.unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(_abi.ConvDesc(n, h, w, cin, cout, cin, cout, prec, dil)))


def _bytes(s, cin, cout, kd=1):
    return 256 + s * kd * 9 * cin * cout * 4


def _tiers(case):
    yield FP32, case.wgrad
    for prec, tier in ((BF16, case.bf16), (BF16S, case.bf16s)):
        if tier is not None:
            yield prec, tier[3]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_query_is_256_bytes_and_whole_slabs_of_the_traced_reducer(L, case):
    """Every row, every precision it admits: the query is 256 bytes + S whole slabs, and S lies in the range of the reducer the
    row's filter-gradient trace names (none: S = 1, <1>: 2 .. 7, <4>: 8 .. 63, <16>: from 64); a refused launch asks for 0."""
    for prec, names in _tiers(case):
        got = _query(L, case.n, case.h, case.w, case.cin, case.cout, prec, case.dil)
        if names is None:
            assert got == 0, (prec, got)
            continue
        slab = 9 * case.cin * case.cout * 4
        assert got > 256 and (got - 256) % slab == 0, (prec, got)
        s = (got - 256) // slab
        red = [n for n in names if n.startswith("slab_reduce")]
        lo, hi = {(): (1, 1), ("slab_reduce_kernel<1>",): (2, 7), ("slab_reduce_kernel<4>",): (8, 63),
                  ("slab_reduce_kernel<16>",): (64, 1 << 30)}[tuple(red)]
        assert lo <= s <= hi, (prec, s, red)


@pytest.mark.parametrize("rid", sorted(WG_PLANS))
def test_query_is_exact_for_the_splits_of_the_table(L, rid):
    c = BY_ID[rid]
    s_fp32, s_bf16, _ = WG_PLANS[rid]
    assert _query(L, c.n, c.h, c.w, c.cin, c.cout, FP32, c.dil) == _bytes(s_fp32, c.cin, c.cout)
    if s_bf16 is not None:
        assert _query(L, c.n, c.h, c.w, c.cin, c.cout, BF16, c.dil) == _bytes(s_bf16, c.cin, c.cout)


def test_atrous_query_rounds_the_wanted_splits_down_as_the_launch_does(L):
    """19 x 18 x 48 pixels in 6 x 16 tiles: 19 x 3 x 3 = 171 tiles; 192 -> 64 channels: 3 panels.  The launch wants
    floor(512 / 3) = 170 splits, so 2 tiles per split and S = ceil(171 / 2) = 86.  (Rounded up, 171 wanted splits would be one
    tile each: S = 171, what the query asked for while it derived the atrous plan a second time.)"""
    assert _query(L, 19, 18, 48, 192, 64, FP32, dil=2) == _bytes(86, 192, 64)
    assert _query(L, 19, 18, 48, 192, 64, BF16, dil=2) == 0          # the atrous tiles are fp32 only: refused, nothing asked


def test_first_layer_3d_query_covers_the_taps_that_run_fewer_planes(L):
    """A (3,3,3), stride-1 first layer, N = 1, D = 8, 96 x 96, 1 -> 32 channels: no fused launch for a first layer, so one
    launch per depth tap.  Depth tap 1 reaches all 8 planes: 8 x 12 x 6 = 576 tiles of 8 x 16, 512 splits wanted -> 2 tiles per
    split -> 288 splits.  Taps 0 and 2 reach 7 planes: 7 x 72 = 504 tiles <= 512 -> one tile per split -> 504 splits, more
    slabs than the launch over every plane takes."""
    from boxsegliver_amd import _abi
    d = _abi.Conv3dDesc(1, 8, 96, 96, 1, 32, 3, 1, 1, 1, 32)
    assert L.unetk_conv3d_ws_bytes(ctypes.byref(d)) >= _bytes(504, 1, 32)


@pytest.mark.parametrize("case", c3.CASES, ids=[c.id for c in c3.CASES])
def test_3d_bf16_query_is_the_plan_of_its_one_launch(L, case):
    """UNETK_BF16 3-D layers run one filter-gradient launch (kd = 3: the depth taps fused, kd slabs per split)."""
    from boxsegliver_amd import _abi
    d = _abi.Conv3dDesc(case.n, case.d, case.h, case.w, case.cin, case.cout, case.kd, 1, 1, case.cin, case.cout)
    assert L.unetk_conv3d_ws_bytes_bf16(ctypes.byref(d)) == _bytes(case.splits, case.cin, case.cout, case.kd)
