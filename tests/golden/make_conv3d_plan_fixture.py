"""Records the host queries of the 3-D conv composition (csrc/conv3d.hip): tests/golden/conv3d_plan_queries.npz.

Run once, at the commit before the queries were moved onto conv3d_plan:  python tests/golden/make_conv3d_plan_fixture.py
It asks whatever library UNETK_LIB names (default: the tree's own).  test_conv3d_plan_host.py imports `groups` and `ask` from
here and holds the library to the recorded values: unetk_conv3d_out_dims, unetk_conv3d_stat_rows, unetk_conv3d_ws_bytes,
unetk_conv3d_stat_rows_bf16 and unetk_conv3d_ws_bytes_bf16 of

  * every case of the extent sweep (conv3d_sweep_cases.ITEMS), the sliced ones with the pixel strides of their wider buffers;
  * every row of conv3d_bf16_cases.CASES;
  * UNet3D's own conv layers (NetworksV2/UNet3D.py model_config / param_specs) at its 96^3 patch and at the reference's
    10 x 256 x 256 training shape, one and two samples, with the live-channel masks of the padded filters and the pixel strides
    of the skip outputs that live in their concat buffers.

All five are pure host arithmetic: no GPU."""
import collections
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv3d_bf16_cases as B  # noqa: E402
import conv3d_sweep_cases as S  # noqa: E402

OUT = os.path.join(HERE, "conv3d_plan_queries.npz")
# a descriptor, field for field (the two masks as one integer each: bit i = channels [8 i, 8 i + 8) are live)
Desc = collections.namedtuple("Desc", "n d h w cin cout kd sd shw xs ys cin_live cout_live")
VALUES = ("rc", "do", "ho", "wo", "stat_rows", "ws_bytes", "stat_rows_bf16", "ws_bytes_bf16")


def _live_mask(phys, segs):
    """NetworksV2/padded.py live8_masks for one axis."""
    m = 0
    if phys % 16 == 0 and phys <= 512:
        for _, ln, ps in segs:
            for g in range(ps // 8, (ps + ln + 7) // 8):
                m |= 1 << g
    return m


def unet3d_layers(n, d, h, w, init_channels=30, num_pool_layers=4, max_channels=320):
    """The conv3d descriptors of one UNet3D forward, in order (NetworksV2/UNet3D.py _build_network)."""
    from boxsegliver_amd.NetworksV2.UNet3D import model_config, param_specs
    from boxsegliver_amd.NetworksV2.padded import pad_to
    specs, pads = param_specs(1, 3, init_channels, num_pool_layers, max_channels, "instance_norm", "UNet3D")
    lshape = {name: shape for name, shape, _ in specs}
    out, enc = [], {}
    cin, xs = 1, 1
    c = init_channels
    for block, layers in model_config(num_pool_layers):
        decoder = block.startswith("conv_d")
        if decoder:
            c, (d, h, w) = enc[block.replace("d", "e")]
            cin = xs = 2 * pad_to(c)                  # concat(skip, up), dense
        pc = pad_to(c)
        for li, (lname, k, stride) in enumerate(layers):
            if lname == "up":
                continue
            wname = "UNet3D/{}/{}/weights".format(block, lname)
            phys, axes = pads[wname]
            assert phys[3] == cin and phys[4] == pc, (wname, phys, cin, pc)
            skip = not decoder and block != "bridge" and li == len(layers) - 1      # written into its decoder concat buffer
            ys = 2 * pc if skip else pc
            out.append(Desc(n, d, h, w, cin, pc, k[0], stride[0], stride[1], xs, ys,
                            _live_mask(phys[3], axes.get(3, [(0, lshape[wname][3], 0)])),
                            _live_mask(phys[4], axes.get(4, [(0, lshape[wname][4], 0)]))))
            d, h, w = -(-d // stride[0]), -(-h // stride[1]), -(-w // stride[2])
            cin, xs = pc, ys
        if not decoder:
            enc[block] = (c, (d, h, w))
            c = min(c * 2, max_channels)
    return out


def groups():
    """Ordered {group name: [Desc]}."""
    g = collections.OrderedDict()
    for item in S.ITEMS:
        g["sweep " + S.item_id(item)] = [
            Desc(c.n, c.d, c.h, c.w, c.cin, c.cout, c.kd, c.stride[0], c.stride[1], c.cin + (S.SLICE_EXTRA if c.sliced else 0),
                 c.cout + (S.SLICE_EXTRA if c.sliced else 0), 0, 0) for c in S.cases(*item)]
    g["bf16 cases"] = [Desc(c.n, c.d, c.h, c.w, c.cin, c.cout, c.kd, 1, 1, c.cin + c.xpad, c.cout + c.ypad, 0, 0) for c in B.CASES]
    g["unet3d 96^3"] = unet3d_layers(1, 96, 96, 96) + unet3d_layers(2, 96, 96, 96)
    g["unet3d 10x256x256"] = unet3d_layers(1, 10, 256, 256) + unet3d_layers(2, 10, 256, 256)
    return g


def c_desc(t):
    from boxsegliver_amd import _abi
    d = _abi.Conv3dDesc(t.n, t.d, t.h, t.w, t.cin, t.cout, t.kd, t.sd, t.shw, t.xs, t.ys)
    for field, m in ((d.cin_live8, t.cin_live), (d.cout_live8, t.cout_live)):
        field[0], field[1] = m & 0xFFFFFFFF, m >> 32
    return d


def library():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_conv3d_ws_bytes", "unetk_conv3d_ws_bytes_bf16"):
        getattr(lib, name).restype = ctypes.c_size_t
    return lib


def ask(lib, t):
    """The VALUES of one descriptor (the output extents stay -1 where unetk_conv3d_out_dims refuses)."""
    d = c_desc(t)
    pd = ctypes.byref(d)
    do, ho, wo = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.unetk_conv3d_out_dims(pd, ctypes.byref(do), ctypes.byref(ho), ctypes.byref(wo))
    return (rc, do.value, ho.value, wo.value, lib.unetk_conv3d_stat_rows(pd), lib.unetk_conv3d_ws_bytes(pd),
            lib.unetk_conv3d_stat_rows_bf16(pd), lib.unetk_conv3d_ws_bytes_bf16(pd))


def main():
    lib = library()
    arrays = {}
    for i, (name, descs) in enumerate(groups().items()):
        arrays["desc_%02d" % i] = np.array(descs, dtype=np.int64)
        arrays["values_%02d" % i] = np.array([ask(lib, t) for t in descs], dtype=np.int64)
    arrays["names"] = np.array(list(groups()))
    np.savez_compressed(OUT, **arrays)
    print("{}: {} descriptors in {} groups, {} bytes".format(OUT, sum(len(v) for k, v in arrays.items() if k.startswith("desc")),
                                                             len(arrays["names"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
