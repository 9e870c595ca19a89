"""UNETK_BF16 for the 3-D convs without a GPU: the layer rule (include/unetk.h) as the library states it through
unetk_conv3d_ws_bytes_bf16 / _stat_rows_bf16, its Python restatement (ops.conv3d_bf16_ok) over UNet3D's layers, and the
argument validation of the new entry points (every refusal is decided on the host, before anything is launched)."""
import ctypes

import pytest

from boxsegliver_amd import _abi, ops
from boxsegliver_amd.NetworksV2.UNet3D import model_config
from boxsegliver_amd.NetworksV2.padded import pad_to

NEW = ("unetk_conv3d_pack_bf16", "unetk_conv3d_stat_rows_bf16", "unetk_conv3d_ws_bytes_bf16", "unetk_conv3d_fwd_bf16",
       "unetk_conv3d_dgrad_bf16", "unetk_conv3d_wgrad_bf16")
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3


def _p(v):
    return ctypes.c_void_p(v)


def unet3d_convs(n=1, d=96, size=96, npl=4, init=30, cap=320):
    """(scope, desc) of every conv3d of UNet3D (NetworksV2/UNet3D.py) at the padded device channel counts."""
    out, c, dd, h = [], init, d, size
    cin, enc = 1, {}
    for block, layers in model_config(npl):
        if block.startswith("conv_e") or block == "bridge":
            for lname, k, stride in layers:
                desc = ops.conv3d_desc((n, dd, h, h, cin), pad_to(c), k[0], stride)
                out.append(("{}/{}".format(block, lname), desc))
                dd, h = -(-dd // stride[0]), -(-h // stride[1])
                cin = pad_to(c)
            enc[block] = (c, dd, h)
            c = min(c * 2, cap)
        else:
            c, dd, h = enc[block.replace("d", "e")]
            cin = 2 * pad_to(c)
            for lname, k, stride in layers:
                if lname == "up":
                    continue
                out.append(("{}/{}".format(block, lname), ops.conv3d_desc((n, dd, h, h, cin), pad_to(c), k[0], stride)))
                cin = pad_to(c)
    return out


def test_new_symbols_are_declared_and_bound():
    lib = _abi.lib()
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.unetk_abi_version() == _abi.ABI_VERSION == 10


def test_layer_rule_over_unet3d_at_96_cubed():
    """13 of the 18 convs run on the bf16 pipe: all but the first conv (Cin = 1) and the four strided convs.  The library
    and ops.conv3d_bf16_ok agree on every layer."""
    lib = _abi.lib()
    convs = unet3d_convs()
    assert len(convs) == 18
    on = [s for s, d in convs if ops.conv3d_bf16_ok(d)]
    off = sorted(s for s, d in convs if not ops.conv3d_bf16_ok(d))
    assert len(on) == 13
    assert off == sorted(["conv_e0/conv1", "conv_e1/conv1", "conv_e2/conv1", "conv_e3/conv1", "bridge/conv1"])
    for s, d in convs:
        ok = ops.conv3d_bf16_ok(d)
        assert (lib.unetk_conv3d_ws_bytes_bf16(ctypes.byref(d)) > 0) == ok, s
        rows = lib.unetk_conv3d_stat_rows_bf16(ctypes.byref(d))
        assert (rows > 0 and rows % d.N == 0) if ok else rows == E_UNSUPPORTED, (s, rows)
        assert ops.conv3d_precision(d, _abi.BF16) == (_abi.BF16 if ok else _abi.FP32)
        assert ops.conv3d_precision(d, _abi.FP32) == _abi.FP32


@pytest.mark.parametrize("shape", [
    # N, D, H, W, Cin, Cout, kd, stride
    (1, 8, 32, 32, 64, 64, 3, (1, 2, 2)),      # strided H / W
    (1, 8, 32, 32, 64, 64, 3, (2, 2, 2)),      # strided depth
    (1, 8, 32, 32, 48, 64, 3, (1, 1, 1)),      # Cin % 32 != 0
    (1, 8, 32, 32, 64, 48, 1, (1, 1, 1)),      # Cout % 32 != 0
    (1, 8, 32, 32, 1, 32, 1, (1, 1, 1)),       # the first conv
])
def test_entry_points_refuse_descriptors_outside_the_rule(shape):
    lib = _abi.lib()
    n, dd, h, w, cin, cout, kd, stride = shape
    d = ops.conv3d_desc((n, dd, h, w, cin), cout, kd, stride)
    assert not ops.conv3d_bf16_ok(d)
    fake, ws = _p(1 << 20), _p(1 << 21)
    big = 1 << 40
    assert lib.unetk_conv3d_ws_bytes_bf16(ctypes.byref(d)) == 0
    assert lib.unetk_conv3d_stat_rows_bf16(ctypes.byref(d)) == E_UNSUPPORTED
    assert lib.unetk_conv3d_fwd_bf16(ctypes.byref(d), fake, fake, fake, None, ws, big, None) == E_UNSUPPORTED
    assert lib.unetk_conv3d_dgrad_bf16(ctypes.byref(d), fake, fake, fake, ws, big, None) == E_UNSUPPORTED
    assert lib.unetk_conv3d_wgrad_bf16(ctypes.byref(d), fake, fake, fake, ws, big, None) == E_UNSUPPORTED
    if cin % 32 or cout % 32:
        assert lib.unetk_conv3d_pack_bf16(fake, kd, cin, cout, fake, fake, None) == E_UNSUPPORTED


def test_entry_points_refuse_a_missing_misaligned_or_short_workspace():
    lib = _abi.lib()
    for kd in (1, 3):
        d = ops.conv3d_desc((2, 4, 24, 24, 128), 128, kd, (1, 1, 1))
        nb = lib.unetk_conv3d_ws_bytes_bf16(ctypes.byref(d))
        assert nb >= 256
        fake = _p(1 << 20)
        calls = (lambda ws, b: lib.unetk_conv3d_fwd_bf16(ctypes.byref(d), fake, fake, fake, None, ws, b, None),
                 lambda ws, b: lib.unetk_conv3d_dgrad_bf16(ctypes.byref(d), fake, fake, fake, ws, b, None),
                 lambda ws, b: lib.unetk_conv3d_wgrad_bf16(ctypes.byref(d), fake, fake, fake, ws, b, None))
        for call in calls:
            assert call(None, nb) == E_BADARG
            assert call(_p((1 << 21) + 8), nb) == E_BADARG
            assert call(_p(1 << 21), nb - 16) == E_WORKSPACE
        # missing operands and invalid descriptors
        assert lib.unetk_conv3d_fwd_bf16(ctypes.byref(d), None, fake, fake, None, _p(1 << 21), nb, None) == E_BADARG
        assert lib.unetk_conv3d_fwd_bf16(None, fake, fake, fake, None, _p(1 << 21), nb, None) == E_BADARG
    bad = ops.conv3d_desc((1, 4, 8, 8, 64), 64, 2, (1, 1, 1))           # kd = 2 is no conv of the model
    assert lib.unetk_conv3d_stat_rows_bf16(ctypes.byref(bad)) == E_BADARG
    assert lib.unetk_conv3d_pack_bf16(None, 3, 64, 64, _p(1 << 20), None, None) == E_BADARG
