"""No GPU: the library's host queries agree with the table of tests/test_gpu_conv_paths.py.

The launch, the statistic-row query and the workspace query of a 3x3 convolution all read one plan (csrc/conv_igemm.hip,
unetk_conv_plan), and the queries are pure host arithmetic, so they can be asked without a device: for every row of CASES the
statistic rows of each precision, which rows want stream-K scratch, and where the fused norm-backward reduction is refused.
Rows with xpad / ypad are asked with the padded pixel strides the GPU test uses.
"""
import ctypes

import pytest

from test_gpu_conv_paths import CASES, FP32, BF16, BF16S

IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def L():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    lib.unetk_conv3x3_ws_bytes.restype = ctypes.c_size_t
    return lib


def _desc(c, prec):
    from boxsegliver_amd import _abi
    pad = prec != BF16S           # the bf16-storage tier runs the rows dense
    return _abi.ConvDesc(c.n, c.h, c.w, c.cin, c.cout, c.cin + (c.xpad if pad else 0), c.cout + (c.ypad if pad else 0), prec, c.dil)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stat_rows_of_every_precision(L, case):
    assert L.unetk_conv3x3_stat_rows(ctypes.byref(_desc(case, FP32))) == case.rows
    for prec, tier in ((BF16, case.bf16), (BF16S, case.bf16s)):
        if tier is not None:
            assert L.unetk_conv3x3_stat_rows(ctypes.byref(_desc(case, prec))) == tier[1], prec


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_workspace_is_asked_exactly_where_stream_k_runs(L, case):
    sk = any("lin_sk_fixup_kernel" in n for names in (case.fwd, case.dgrad) if names for n in names)
    assert (L.unetk_conv3x3_ws_bytes(ctypes.byref(_desc(case, FP32))) > 0) == sk


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_fused_reduction_where_the_input_gradient_is_refused_or_linear(L, case):
    if case.dgrad is None or "conv3x3_igemm_lin_kernel" in case.dgrad[0]:
        assert L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(_desc(case, FP32))) == 0


def test_unpadded_30_channel_3d_layer_asks_for_no_stream_k_scratch(L):
    """Found while the queries were moved onto the plan: for a 3-D layer with 30 (not 32) channels on small planes the workspace
    query used to test the linear-pixel kernel's admission with the LIVE channel count rounded to 16-channel chunks (16) in place
    of Cin = 30, and asked for a stream-K slab (9437184 bytes here) that no launch takes: the forward runs the first-layer
    kernel and the gradients refuse the channel count.  The query now follows the launch."""
    from boxsegliver_amd import _abi
    L.unetk_conv3d_ws_bytes.restype = ctypes.c_size_t
    d = _abi.Conv3dDesc(1, 1, 96, 24, 30, 512, 1, 1, 1, 30, 512)
    assert L.unetk_conv3d_ws_bytes(ctypes.byref(d)) == 0
    d = _abi.Conv3dDesc(1, 1, 96, 24, 32, 512, 1, 1, 1, 32, 512)
    assert L.unetk_conv3d_ws_bytes(ctypes.byref(d)) > 0
