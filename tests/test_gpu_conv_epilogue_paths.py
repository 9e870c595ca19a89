"""The fused epilogues of the 3x3 convolution family on every dispatch path, with inputs for which fp32 and bf16 arithmetic are
exact: the inference epilogue (unetk_conv3x3_fwd_affine: conv + (scale, shift) + ReLU [+ 2 x 2 max-pool] in one pass) and the
input gradient fused with the producer's norm-backward reduction (unetk_conv3x3_dgrad_nbr, ops.FUSE_NBR).

The convolution operands are those of test_gpu_conv_paths.py (x integers in [-4, 4], w eighths in [-2/8, 2/8], dy integers in
[-2, 2]), so every accumulator equals the float64 convolution whatever the tile, split or MFMA order; each row asserts that
bound from its own inputs.  On top of that:

  affine  scale in +-{1/2, 1, 2} (one channel in five negative), shift multiples of 1/8 in [-2, 2]: fmaf(acc, scale, shift) is
          exact, so z must equal float64 relu(conv * scale + shift) bit for bit (under UNETK_BF16S: that value rounded ONCE to
          bf16, nearest even), and `pooled` the 2 x 2 maximum of that REFERENCE -- not merely of the kernel's own z.  z goes into
          a channel slice (offset 32) of a buffer 64 channels wider, pooled into one with its own stride (Cout + 32); the guard
          bands and the neighbour channels must stay bit-unchanged and every element of the views written.
  NBR     prod_y integers in [-4, 4] (in the storage dtype), mean in {-1, 0, 1}, rstd in {1/2, 1, 2}, scale in +-{1/2, 1, 2},
          shift multiples of 1/2 in [-2, 2]; with per_sample = 1 the four tables differ from sample to sample.  dx must equal
          the float64 transposed convolution bit for bit (bf16 storage: rounded once) and, under bf16 storage, du is built from
          the STORED dx ("on the values memory holds").  du and du * xhat are multiples of 1/8 and 1/16; each row asserts that
          the largest sum of |du * xhat| * 16 and of |du| * 8 over one tile's pixels stays below 2^24, so any summation order
          inside a tile is exact, and the partial rows of each sample (rows % N == 0, contiguous), summed in float64, must
          equal the reference exactly for k = 0 and k = 1.

Both references take the mask as `> 0`.  Every row asserts that it has ties (pre-activation exactly 0) and negative
pre-activations, and the NBR rows that a reference with `>= 0` gives other sums, so the row tells the two apart; the bf16-storage
NBR rows assert the same of a du built from the unrounded accumulators.  Measured share of ties, exact tier: NBR 6.7 .. 7.7 %
of the elements at exactly 0 and 52 .. 56 % masked (max |dx| 42 .. 65: above 32 an odd eighth does not fit bf16, so the store is
a real rounding, asserted per row); the largest per-tile sums reach 1.6 % of 2^24.  Affine: 0.09 % (Cin = 1024) .. 1.8 %
(Cin = 1) at exactly 0, 46 .. 57 % negative.  Gaussian tier: no ties (not asserted there).

Each row names the kernel it exists to reach and the library's launch trace must show exactly that (test_gpu_conv_paths._trace).
The rows were chosen by reading plan_dense / small_grid / big_grid (csrc/conv_igemm.hip), unetk_conv_plan_lin / sk_plan
(csrc/conv_igemm_lin.hip), pick_bf16 / unetk_conv_plan_bf16 (csrc/conv_igemm_bf16.hip) and unetk_conv_plan_bf16s_v3
(csrc/conv_igemm_bf16s.hip); tests/test_conv_epilogue_paths_host.py asks the host queries for the same table without a device.

Instantiations no admissible shape reaches: none of those the entry points can launch.  (conv3x3_igemm_kernel<4,1,*,*,1,1,2>
does not exist: the fused reduction is for the 128-wide tiles, and launch_igemm instantiates MODE 2 for WN == 2 only; narrower
dx tiles are refused by unetk_conv3x3_dgrad_nbr_rows.  conv3x3_bf16s_kernel<4,true,0> is never launched either: the persistent
kernel's reduction exists for its 128-wide tile, and dx channels are a multiple of 128 wherever the fused variant is offered.)

Gaussian tier, the project's bounds unchanged: fp32 z 2e-6 and dx 3e-6 of the output's range, partials 1e-5 against the float64
reduction of the device's own dx (test_gpu_guard_bands.py::test_conv3x3_dgrad_nbr_edges); bf16 storage: stored values within
one bf16 ulp of the exact result and all but 2e-3 of them its exact rounding (_stored_ok).  One row cannot hold 2e-6 for fp32
arithmetic alone and carries the rule of test_gpu_head.py's header (4 x the error of the same operation in torch float32 on the
CPU against float64 on that row's Gaussian inputs): aff_sk_nc48 (Cin = 768; the 256 whole tiles of its stream-K launch run their
K = 6912 loop in one fp32 chain; the exact tier shows this very launch bit-equal to float64).  Measured: CPU float32 3.16e-6, the
kernel's own 3.57e-6 (GAUSS_Z_TOL).  The other stream-K rows hold 2e-6 (the kernel 4.8e-7 .. 7.4e-7).

Small rows take the float64 convolution from oracle/tf_ops.conv_nd_same on the CPU, the others from the same function on the
device.  The reference of a row is computed once and shared by its variants (pool off / on, per_sample 0 / 1).
"""
import collections
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import tf_ops
import guardbuf
from test_gpu_conv_paths import ops  # noqa: F401  (the module-scoped fixture)
from test_gpu_conv_paths import (CASES, FP32, BF16, BF16S, PREC_NAME, E_BADARG, E_UNSUPPORTED, lib, _p, _stream, _trace,
                                 _assert_trace, _stored_ok, _r)

pytestmark = pytest.mark.gpu

IG, LINK, BFK, V3, C3 = "conv3x3_igemm_kernel", "conv3x3_igemm_lin_kernel", "conv3x3_igemm_bf16_kernel", "conv3x3_bf16s_kernel", "conv3x3_c3_mfma_kernel"

# ---------------------------------------------------------------------------------------------------------------- the tables
# NBR: descriptor (N, H, W, Cin = dx channels, Cout = dy channels), precision, partial rows, tile height of the kernel, the
# kernel, prod_y pixel stride beyond Cin (pys), and the statistic rows of the FORWARD conv of the same descriptor (frows: what
# unetk_conv3x3_stat_rows answers; asked by the host module).
Nbr = collections.namedtuple("Nbr", "id n h w cin cout prec rows th kern pys frows plain")


def _n(id, n, h, w, cin, cout, prec, rows, th, kern, frows, pys=0, plain=None):
    return Nbr(id, n, h, w, cin, cout, prec, rows, th, kern, pys, frows, plain)


NBR_ROWS = [
    # 2 x 6 x 3 tiles of 4 x 16 pixels: H = 22 and W = 40 leave the last tile row / column ragged
    _n("nbr_t4", 2, 22, 40, 128, 128, FP32, 36, 4, IG + "<2,2,1,2,1,1,2>", 36),
    # 8 x 6 x 5 x 2 = 480 blocks: past small_grid's 384; H % 16 != 0 keeps the 8-row tile
    _n("nbr_t8", 8, 44, 72, 256, 128, FP32, 240, 8, IG + "<2,2,2,2,1,1,2>", 440),
    # 8 x 4 x 8 x 2 = 512 blocks of 16 rows: the plain input gradient takes the 16-row tile, the fused one (128 contraction
    # channels < 256) the 8-row tile
    _n("nbr_t8_k128", 8, 64, 120, 256, 128, FP32, 512, 8, IG + "<2,2,2,2,1,1,2>", 512, plain=IG + "<2,2,4,2,1,1,0>"),
    _n("nbr_t16", 8, 64, 120, 256, 256, FP32, 256, 16, IG + "<2,2,4,2,1,1,2>", 256),
    # H < 24: pick_bf16 cfg 1, 8-row tiles
    _n("nbr_bs128", 2, 20, 40, 128, 128, BF16S, 18, 8, BFK + "<2,2,2,2,true,true,false>", 18),
    # 6 x 2 x 13 x 4 = 624 tiles of 32 x 16 pixels x 128 channels on at most 256 resident blocks: each walks >= 2 tiles
    _n("nbr_bs_v3", 6, 40, 200, 512, 128, BF16S, 156, 32, V3 + "<8,true,0>", 390),
    # prod_y_stride % 8 != 0: the persistent kernel cannot read 16-byte rows of it, the tall tile emits the same rows
    _n("nbr_bs_tall", 6, 40, 200, 512, 128, BF16S, 156, 32, BFK + "<4,2,4,2,true,true,false>", 390, pys=4),
]
NBR_BY_ID = {r.id: r for r in NBR_ROWS}
# also run with prod_y a channel slice of a wider buffer, row id -> (channels beyond Cin, channel offset): stride Cin + 64 at
# offset 32, and the least aligned views include/unetk.h admits -- fp32 scalars at an odd stride and offset, the tall bf16 tile's
# 4-byte words at a base that is a multiple of 4 bytes only
NBR_SLICED = [("nbr_t4", 64, 32), ("nbr_bs128", 64, 32), ("nbr_t4", 3, 1), ("nbr_bs_tall", 4, 2)]
# (what, descriptor, precision): unetk_conv3x3_dgrad_nbr_rows = 0 and the entry point returns UNETK_E_UNSUPPORTED
NBR_REFUSED = [
    ("UNETK_BF16", (2, 22, 40, 128, 128), BF16),
    ("dx channels % 128", (2, 22, 40, 64, 128), FP32),
    ("dy channels < 128", (2, 22, 40, 128, 64), FP32),
    ("linear-pixel plane", (2, 16, 16, 128, 128), FP32),
]

# affine: descriptor, precision, statistic rows of the plain forward of the shape (host module), kernels ("{m}" = 3 without,
# 4 with the pool; for the persistent kernel 1 / 2), pool admitted, the whole row admitted
Aff = collections.namedtuple("Aff", "id n h w cin cout prec rows kern pool ok")


def _a(id, n, h, w, cin, cout, rows, kern, pool=True, prec=FP32, ok=True):
    return Aff(id, n, h, w, cin, cout, prec, rows, kern if isinstance(kern, list) or kern is None else [kern], pool, ok)


_SK_ROWS = [c for c in CASES if any("lin_sk_fixup_kernel" in k for k in c.fwd)]      # sk128, sk64, sk128x64, sk_t256, sk_nc48, lin_starved256
AFF_ROWS = [
    _a("aff_t4", 2, 22, 40, 32, 128, 36, IG + "<2,2,1,2,1,1,{m}>"),               # H = 22: the last 4-row tile holds one window row
    _a("aff_t8", 8, 44, 72, 32, 256, 240, IG + "<2,2,2,2,1,1,{m}>"),
    _a("aff_t16", 8, 64, 120, 16, 256, 256, IG + "<2,2,4,2,1,1,{m}>"),
    _a("aff_n64", 2, 20, 40, 32, 64, 18, IG + "<4,1,1,2,1,1,{m}>"),
    _a("aff_n64_t16", 8, 128, 120, 16, 64, 512, IG + "<4,1,2,2,1,1,{m}>"),
    _a("aff_n32_co32", 2, 24, 40, 16, 32, 12, IG + "<4,1,2,1,1,1,{m}>"),
    _a("aff_n32_co96", 2, 24, 40, 16, 96, 12, IG + "<4,1,2,1,1,1,{m}>"),
    _a("aff_lin64", 1, 8, 16, 64, 128, 2, LINK + "<2,2,1,2,false,false,false,false,false,false>", pool=False),
    _a("aff_lin128x64", 2, 24, 20, 32, 64, 8, LINK + "<4,1,1,2,false,false,false,false,false,false>", pool=False),
    _a("aff_lin_sk", 8, 16, 16, 128, 128, 16,
       [LINK + "<2,2,2,2,false,false,true,false,false,false>", "lin_sk_fixup_kernel<128,128>"], pool=False),
] + [
    _a("aff_" + c.id, c.n, c.h, c.w, c.cin, c.cout, c.rows, list(c.fwd), pool=False) for c in _SK_ROWS
] + [
    _a("aff_c3_ci%d" % ci, 2, 24, 40, ci, 64, 18, C3 + "<%d,float,true>" % ci, pool=False) for ci in (1, 2, 3, 4, 5)
] + [
    _a("aff_c3_ci%d_bs" % ci, 2, 24, 40, ci, 64, 18, C3 + "<%d,unsignedshort,true>" % ci, pool=False, prec=BF16S) for ci in (1, 2, 3, 4, 5)
] + [
    _a("aff_bs_v3_128", 4, 40, 200, 64, 256, 104, V3 + "<8,false,{m}>", prec=BF16S),      # 4 x 2 x 13 x 2 = 208 tiles
    _a("aff_bs_v3_64", 8, 40, 200, 64, 64, 208, V3 + "<4,false,{m}>", prec=BF16S),        # 8 x 2 x 13 = 208 tiles
    # refused: the inference epilogue of the bf16-storage mode lives in the persistent kernel only (18 tiles here); the
    # first-layer kernel has it for Cout = 64 and Cin <= 5
    _a("aff_bs_small", 2, 20, 40, 64, 128, 18, None, pool=False, prec=BF16S, ok=False),
    _a("aff_c3_ci6", 2, 24, 40, 6, 64, 18, None, pool=False, ok=False),
    _a("aff_c3_co32", 2, 24, 40, 3, 32, 18, None, pool=False, ok=False),
    _a("aff_c3_ci6_bs", 2, 24, 40, 6, 64, 18, None, pool=False, prec=BF16S, ok=False),
]
AFF_BY_ID = {r.id: r for r in AFF_ROWS}
# the pool on odd extents is refused whatever the kernel: (N, H, W, Cin, Cout, precision)
AFF_ODD_POOL = [(2, 21, 40, 32, 128, FP32), (2, 22, 39, 32, 128, FP32), (4, 40, 199, 64, 256, BF16S)]

REQUIRED = (
    [IG + "<%s,1,1,%d>" % (t, m) for t in ("2,2,1,2", "2,2,2,2", "2,2,4,2", "4,1,1,2", "4,1,2,2", "4,1,2,1") for m in (3, 4)]
    + [LINK + "<2,2,1,2,false,false,false,false,false,false>", LINK + "<4,1,1,2,false,false,false,false,false,false>",
       LINK + "<2,2,2,2,false,false,true,false,false,false>", LINK + "<2,2,1,2,false,false,true,false,false,false>",
       LINK + "<4,1,1,2,false,false,true,false,false,false>",
       "lin_sk_fixup_kernel<64,128>", "lin_sk_fixup_kernel<128,128>", "lin_sk_fixup_kernel<128,64>"]
    + [C3 + "<%d,%s,true>" % (ci, t) for ci in (1, 2, 3, 4, 5) for t in ("float", "unsignedshort")]
    + [V3 + "<%d,false,%d>" % (nt, m) for nt in (4, 8) for m in (1, 2)]
    + [IG + "<2,2,1,2,1,1,2>", IG + "<2,2,2,2,1,1,2>", IG + "<2,2,4,2,1,1,2>",
       BFK + "<4,2,4,2,true,true,false>", BFK + "<2,2,2,2,true,true,false>", V3 + "<8,true,0>"])

# Gaussian tier, z bound where fp32 arithmetic alone exceeds 2e-6: 4 x the error of relu(conv * scale + shift) evaluated in
# torch float32 on the CPU against float64 on the row's own Gaussian inputs (measured there: 3.165e-6)
GAUSS_Z_TOL = {"aff_sk_nc48": 4 * 3.165e-6}

TRACED = {}        # (row id, variant) -> traced names of the exact tier
_REF = {}          # the last row's float64 convolution: (row id, kind) -> tensor on the device


def _cd(a, b):
    return -(-a // b)


def _seed(rid, kind):
    return 9100 + sum(ord(ch) for ch in rid) + (0 if kind == "exact" else 1)


def _desc(r, xs=None, ys=None):
    from boxsegliver_amd import _abi
    return _abi.ConvDesc(r.n, r.h, r.w, r.cin, r.cout, xs or r.cin, ys or r.cout, r.prec, 1)


def _sd(prec):
    return torch.bfloat16 if prec == BF16S else torch.float32


def _signed_pow2(shape, g):
    """+-{1/2, 1, 2}, about one in five negative."""
    mag = 2.0 ** torch.randint(-1, 2, shape, generator=g).float()
    return torch.where(torch.rand(shape, generator=g) < 0.2, -mag, mag)


def _conv64(key, big, a, w):
    """float64 SAME conv of a [N,H,W,Ci] with w [3,3,Ci,Co], on the device for the big rows; the last result is kept."""
    if key not in _REF:
        _REF.clear()
        dev = "cuda" if big else "cpu"
        _REF[key] = tf_ops.conv_nd_same(a.to(dev).double(), w.to(dev).double()).cuda()
    return _REF[key]


def _is_big(r):
    return r.n * r.h * r.w * max(r.cin, r.cout) > 100000


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------- NBR
def nbr_inputs(r, per_sample, kind):
    """CPU float32 dy, w, prod_y (shared by per_sample 0 / 1) and the tables scale, shift, mean, rstd [N or 1, Cin]."""
    g = torch.Generator().manual_seed(_seed(r.id.replace("_tall", "_v3"), kind))
    t = r.n if per_sample else 1
    ds, ws, ps = (r.n, r.h, r.w, r.cout), (3, 3, r.cin, r.cout), (r.n, r.h, r.w, r.cin)
    if kind == "exact":
        dy = torch.randint(-2, 3, ds, generator=g).float()
        w = torch.randint(-2, 3, ws, generator=g).float() / 8
        py = torch.randint(-4, 5, ps, generator=g).float()
        g2 = torch.Generator().manual_seed(_seed(r.id, kind) + 17 * (1 + per_sample))
        scale = _signed_pow2((t, r.cin), g2)
        shift = torch.randint(-4, 5, (t, r.cin), generator=g2).float() / 2
        mean = torch.randint(-1, 2, (t, r.cin), generator=g2).float()
        rstd = 2.0 ** torch.randint(-1, 2, (t, r.cin), generator=g2).float()
    else:
        dy = torch.randn(ds, generator=g)
        w = torch.randn(ws, generator=g) / (9 * r.cout) ** 0.5
        py = torch.randn(ps, generator=g)
        if r.prec == BF16S:                      # what the kernel is given / rounds its filter to
            dy, w, py = dy.bfloat16().float(), w.bfloat16().float(), py.bfloat16().float()
        g2 = torch.Generator().manual_seed(_seed(r.id, kind) + 17 * (1 + per_sample))
        sgn = torch.where(torch.rand((t, r.cin), generator=g2) < 0.2, -1.0, 1.0)
        scale = sgn * (torch.rand((t, r.cin), generator=g2) + 0.5)
        shift = torch.randn((t, r.cin), generator=g2) * 0.1
        mean = torch.randn((t, r.cin), generator=g2) * 0.1
        rstd = torch.rand((t, r.cin), generator=g2) + 0.5
    return dy, w, py, (scale, shift, mean, rstd)


def _tile_max(a, th):
    """Largest sum of a (>= 0, [N,H,W,C]) over the pixels of one th x 16 tile and one channel."""
    n, h, w, c = a.shape
    hp, wp = _cd(h, th) * th, _cd(w, 16) * 16
    a = F.pad(a, (0, 0, 0, wp - w, 0, hp - h))
    return a.view(n, hp // th, th, wp // 16, 16, c).sum((2, 4)).max().item()


def run_nbr(ops, r, per_sample, kind, sliced=None):
    L = lib()
    sd = _sd(r.prec)
    dy, w, py, tabs = nbr_inputs(r, per_sample, kind)
    d = _desc(r)
    rows = L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(d))
    assert rows == r.rows and rows % r.n == 0 and rows // r.n == _cd(r.h, r.th) * _cd(r.w, 16), (rows, r.rows)
    _, wp_d = ops.conv3x3_pack(w.cuda(), bf16=r.prec)
    pys, coff = (r.cin + sliced[0], sliced[1]) if sliced else (r.cin + r.pys, 0)
    gdy = guardbuf.guarded_input(dy.cuda().to(sd))
    gpy = guardbuf.guarded_input(py.cuda().to(sd), pys, coff)
    gt = [guardbuf.guarded_input(t.cuda()) for t in tabs]
    gdx, gpart = guardbuf.guarded((r.n, r.h, r.w, r.cin), sd), guardbuf.guarded((2, rows, r.cin))
    rc, names = _trace(ops, lambda: L.unetk_conv3x3_dgrad_nbr(
        ctypes.byref(d), _p(gdy.ptr()), _p(wp_d), _p(gdx.ptr()), _p(gpy.ptr()), pys, _p(gt[0].ptr()), _p(gt[1].ptr()),
        _p(gt[2].ptr()), _p(gt[3].ptr()), per_sample, _p(gpart.ptr()), _stream()))
    tag = "{} per_sample={} {}{}".format(r.id, per_sample, kind, " sliced +{} @{}".format(*sliced) if sliced else "")
    assert rc == 0, (tag, rc)
    _assert_trace(names, [r.kern], tag)
    for nm, gb in (("dx", gdx), ("partials", gpart)):
        assert gb.changed_outside() == 0 and gb.unwritten() == 0, (tag, nm, gb.changed_outside(), gb.unwritten())
    for gb in [gdy, gpy] + gt:
        assert gb.changed_anywhere() == 0, tag

    dx = gdx.view.contiguous()
    part = gpart.view.double()
    dx64 = _conv64((r.id.replace("_tall", "_v3"), kind), _is_big(r), dy, w.flip(0, 1).transpose(2, 3))
    py64 = py.cuda().double()
    sc, sh, mu, rs = [t.cuda().double().view(-1, 1, 1, r.cin) for t in tabs]
    pre = py64 * sc + sh
    xhat = (py64 - mu) * rs
    if kind == "gauss":
        if r.prec == BF16S:
            _stored_ok(dx, dx64, tag + " dx")
        else:
            e = _rel(dx, dx64)
            print(tag, "dx", e)
            assert e < 3e-6, e
        du = dx.double() * (pre > 0)                 # the device's own dx: test_conv3x3_dgrad_nbr_edges's rule
        p = part.sum(1)
        e0, e1 = _rel(p[0], du.sum((0, 1, 2))), _rel(p[1], (du * xhat).sum((0, 1, 2)))
        print(tag, "partials", e0, e1)
        assert e0 < 1e-5 and e1 < 1e-5, (e0, e1)
        return
    TRACED.setdefault((r.id, per_sample), set()).update(names)
    # ---- the exact regime, from the row's own inputs
    amax = 9 * r.cout * dy.abs().max().item() * w.abs().max().item()      # >= max(|dy| conv |w|); every partial sum a multiple of 1/8
    assert amax * 8 < 2 ** 24, amax
    assert torch.equal(dx64.float().double(), dx64)
    if r.prec == BF16S:
        stored = _r(dx64)
        assert not torch.equal(stored, dx64), tag + ": the bf16 store rounds nothing"
        assert torch.equal(dx, dx64.float().bfloat16()), tag + " dx"
    else:
        stored = dx64
        assert dx.dtype == torch.float32 and torch.equal(dx.double(), dx64), tag + " dx"
    du = stored * (pre > 0)
    s0, s1 = _tile_max(du.abs(), r.th) * 8, _tile_max((du * xhat).abs(), r.th) * 16
    ties, masked = (pre == 0).double().mean().item(), (pre <= 0).double().mean().item()
    print(tag, "ties", ties, "masked", masked, "max|dx|", dx64.abs().max().item(), "of 2^24:", s0 / 2 ** 24, s1 / 2 ** 24)
    assert s0 < 2 ** 24 and s1 < 2 ** 24, (s0, s1)
    assert ties > 0.01 and bool((pre < 0).any()), (ties, masked)
    want0, want1 = du.sum((1, 2)), (du * xhat).sum((1, 2))
    du_ge = stored * (pre >= 0)
    assert not torch.equal(du_ge.sum((1, 2)), want0) and not torch.equal((du_ge * xhat).sum((1, 2)), want1)
    if r.prec == BF16S:                                  # ... and from a du built on the unrounded accumulators
        du_acc = dx64 * (pre > 0)
        assert not torch.equal(du_acc.sum((1, 2)), want0) and not torch.equal((du_acc * xhat).sum((1, 2)), want1)
    if per_sample:                                       # the tables do differ between the samples
        assert all(not torch.equal(t[0], t[1]) for t in tabs)
    got = part.view(2, r.n, rows // r.n, r.cin).sum(2)
    assert torch.equal(got[0], want0), (tag + " sum du", (got[0] - want0).abs().max().item())
    assert torch.equal(got[1], want1), (tag + " sum du xhat", (got[1] - want1).abs().max().item())


NBR_PARAMS = [(r, ps, None) for r in NBR_ROWS for ps in (0, 1)] + [(NBR_BY_ID[i], 1, (a, b)) for i, a, b in NBR_SLICED]


def _nbr_id(p):
    return "{}-ps{}{}".format(p[0].id, p[1], "-sliced{}at{}".format(*p[2]) if p[2] else "")


@pytest.mark.parametrize("row,per_sample,sliced", NBR_PARAMS, ids=[_nbr_id(p) for p in NBR_PARAMS])
def test_dgrad_nbr_exact(ops, row, per_sample, sliced):
    run_nbr(ops, row, per_sample, "exact", sliced)


@pytest.mark.parametrize("row", NBR_ROWS, ids=[r.id for r in NBR_ROWS])
def test_dgrad_nbr_gaussian(ops, row):
    run_nbr(ops, row, 0, "gauss")


def test_plain_dgrad_of_nbr_t8_k128_takes_the_16_row_tile(ops):
    """big_grid refuses the fused reduction below 256 contraction channels; the plain input gradient of the shape does not."""
    r = NBR_BY_ID["nbr_t8_k128"]
    dy = torch.zeros((r.n, r.h, r.w, r.cout), device="cuda")
    _, wp_d = ops.conv3x3_pack(torch.zeros((3, 3, r.cin, r.cout), device="cuda"))
    _, names = _trace(ops, lambda: ops.conv3x3_dgrad(dy, wp_d, r.cin))
    _assert_trace(names, [r.plain], r.id + " plain")


def _nbr_call(L, ops, shape, prec, py_off=0, pys_extra=0):
    """unetk_conv3x3_dgrad_nbr on zero-filled, full-size operands; prod_y moved by py_off BYTES.  Returns (rc, trace, outputs)."""
    n, h, w, cin, cout = shape
    from boxsegliver_amd import _abi
    d = _abi.ConvDesc(n, h, w, cin, cout, cin, cout, prec, 1)
    sd = _sd(prec)
    pys = cin + pys_extra
    dy = torch.zeros((n, h, w, cout), dtype=sd, device="cuda")
    wp = torch.zeros(9 * cin * cout, dtype=sd, device="cuda")
    py = torch.zeros(n * h * w * pys + 64, dtype=sd, device="cuda")
    tab = torch.ones((n, cin), device="cuda")
    dx = torch.full((n, h, w, cin), 3.0, dtype=sd, device="cuda")
    part = torch.full((2, max(1, n * _cd(h, 4) * _cd(w, 16)), cin), 3.0, device="cuda")
    rc, names = _trace(ops, lambda: L.unetk_conv3x3_dgrad_nbr(
        ctypes.byref(d), _p(dy), _p(wp), _p(dx), _p(py.data_ptr() + py_off), pys, _p(tab), _p(tab), _p(tab), _p(tab), 1,
        _p(part), _stream()))
    return rc, names, (dx, part)


@pytest.mark.parametrize("what,shape,prec", NBR_REFUSED, ids=[r[0] for r in NBR_REFUSED])
def test_dgrad_nbr_refused_shapes(ops, what, shape, prec):
    L = lib()
    from boxsegliver_amd import _abi
    assert L.unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(_abi.ConvDesc(*(shape + (shape[3], shape[4], prec, 1))))) == 0
    rc, names, outs = _nbr_call(L, ops, shape, prec)
    assert rc == E_UNSUPPORTED and names == [], (what, rc, names)
    assert all(bool((o == 3.0).all()) for o in outs)


NBR_MISALIGNED = [
    # what, row whose shape is used, byte offset of prod_y, prod_y stride beyond Cin
    ("fp32 base % 4", "nbr_t4", 2, 0),
    ("bf16 tile base % 4", "nbr_bs128", 2, 0),
    ("bf16 tile odd stride", "nbr_bs128", 0, 1),
    ("persistent kernel base % 16", "nbr_bs_v3", 4, 0),
    ("persistent kernel base % 16 (8)", "nbr_bs_v3", 8, 0),
    ("tall tile base % 4", "nbr_bs_tall", 2, 4),
    ("tall tile odd stride", "nbr_bs_tall", 0, 3),
]


@pytest.mark.parametrize("what,rid,off,extra", NBR_MISALIGNED, ids=[m[0] for m in NBR_MISALIGNED])
def test_dgrad_nbr_refuses_a_prod_y_its_kernel_cannot_read(ops, what, rid, off, extra):
    """include/unetk.h: the fp32 tile reads prod_y as scalars, the bf16 tiles in 4-byte words (even stride), the persistent
    kernel in 16-byte rows.  UNETK_E_BADARG before any launch: an empty trace, outputs untouched."""
    r = NBR_BY_ID[rid]
    rc, names, outs = _nbr_call(lib(), ops, (r.n, r.h, r.w, r.cin, r.cout), r.prec, py_off=off, pys_extra=extra)
    assert rc == E_BADARG and names == [], (what, rc, names)
    assert all(bool((o == 3.0).all()) for o in outs)


# ---------------------------------------------------------------------------------------------------------------- affine
def aff_inputs(r, kind):
    g = torch.Generator().manual_seed(_seed(r.id, kind))
    xs, ws = (r.n, r.h, r.w, r.cin), (3, 3, r.cin, r.cout)
    if kind == "exact":
        x = torch.randint(-4, 5, xs, generator=g).float()
        w = torch.randint(-2, 3, ws, generator=g).float() / 8
        scale = _signed_pow2((r.cout,), g)
        shift = torch.randint(-16, 17, (r.cout,), generator=g).float() / 8
    else:
        x = torch.randn(xs, generator=g)
        w = torch.randn(ws, generator=g) / (9 * r.cin) ** 0.5
        if r.prec == BF16S and r.cin % 16 == 0:          # bf16 activations in, the filter rounded to bf16 by the pack (the
            x, w = x.bfloat16().float(), w.bfloat16().float()      # first-layer kernel multiplies its fp32 image in fp32)
        sgn = torch.where(torch.rand((r.cout,), generator=g) < 0.2, -1.0, 1.0)
        scale = sgn * (torch.rand((r.cout,), generator=g) + 0.5)
        shift = torch.randn((r.cout,), generator=g) * 0.1
    return x, w, scale, shift


def _pool64(z):
    n, h, w, c = z.shape
    return z.view(n, h // 2, 2, w // 2, 2, c).amax((2, 4))


def run_aff(ops, r, pool, kind, use_ws=True):
    L = lib()
    sd = _sd(r.prec)
    first = not (r.cin % 16 == 0 and r.cout % 32 == 0)
    x, w, scale, shift = aff_inputs(r, kind)
    ys, ps = r.cout + 64, r.cout + 32
    d = _desc(r, ys=ys)
    assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 1 if pool else 0) == 1
    wsrc = w.cuda() if first else ops.conv3x3_pack(w.cuda(), want_dgrad=False, bf16=r.prec)[0]
    gx = guardbuf.guarded_input(x.cuda().to(torch.float32 if first else sd))
    gsc, gsh = guardbuf.guarded_input(scale.cuda()), guardbuf.guarded_input(shift.cuda())
    gz = guardbuf.guarded((r.n, r.h, r.w, r.cout), sd, ys, 32)
    gp = guardbuf.guarded((r.n, r.h // 2, r.w // 2, r.cout), sd, ps, 0) if pool else None
    L.unetk_conv3x3_ws_bytes.restype = ctypes.c_size_t
    nws = L.unetk_conv3x3_ws_bytes(ctypes.byref(d)) if use_ws else 0
    ws = guardbuf.GuardedWorkspace(nws)
    ws.fill(0xFF)
    rc, names = _trace(ops, lambda: L.unetk_conv3x3_fwd_affine(
        ctypes.byref(d), _p(gx.ptr()), _p(wsrc), _p(gsc.ptr()), _p(gsh.ptr()), _p(gz.ptr()), _p(gp.ptr()) if pool else None,
        ps if pool else 0, _p(ws.ptr()) if nws else None, ctypes.c_size_t(nws), _stream()))
    tag = "{} pool={} {}{}".format(r.id, int(pool), kind, "" if use_ws else " no ws")
    assert rc == 0, (tag, rc)
    expect = [k.format(m=(2 if pool else 1) if k.startswith(V3) else (4 if pool else 3)) for k in r.kern]
    if not use_ws:
        expect = [expect[0].replace("false,false,true,", "false,false,false,")]
    _assert_trace(names, expect, tag)
    for nm, gb in (("z", gz), ("pooled", gp)):
        if gb is not None:
            assert gb.changed_outside() == 0 and gb.unwritten() == 0, (tag, nm, gb.changed_outside(), gb.unwritten())
    for gb in (gx, gsc, gsh):
        assert gb.changed_anywhere() == 0, tag
    assert ws.guard_intact(), tag

    z = gz.view.contiguous()
    y64 = _conv64((r.id, kind), _is_big(r), x, w)
    pre = y64 * scale.cuda().double() + shift.cuda().double()
    z64 = pre.clamp_min(0)
    if kind == "gauss":
        if r.prec == BF16S:
            _stored_ok(z, z64, tag + " z")
            if pool:
                _stored_ok(gp.view, _pool64(z64), tag + " pooled")
        else:
            e = _rel(z, z64)
            print(tag, "z", e)
            assert e < GAUSS_Z_TOL.get(r.id, 2e-6), e
            if pool:
                assert _rel(gp.view, _pool64(z64)) < 2e-6
        if pool:
            assert torch.equal(gp.view, _pool64(z))
        return z
    TRACED.setdefault((r.id, pool), set()).update(names)
    amax = 9 * r.cin * x.abs().max().item() * w.abs().max().item()        # >= max(|x| conv |w|); partial sums multiples of 1/8
    assert amax * 8 < 2 ** 24, amax
    assert torch.equal(y64.float().double(), y64) and torch.equal(pre.float().double(), pre)
    ties = (pre == 0).double().mean().item()
    print(tag, "ties", ties, "negative", (pre < 0).double().mean().item())
    assert bool((pre == 0).any()) and bool((pre < 0).any()), tag
    if r.prec == BF16S:
        assert z.dtype == torch.bfloat16 and torch.equal(z, z64.float().bfloat16()), tag + " z"
        if pool:
            assert torch.equal(gp.view, _pool64(z64).float().bfloat16()), tag + " pooled"
    else:
        assert z.dtype == torch.float32 and torch.equal(z.double(), z64), tag + " z"
        if pool:
            assert torch.equal(gp.view.double(), _pool64(z64)), tag + " pooled"
    return z


AFF_PARAMS = [(r, pool) for r in AFF_ROWS if r.ok for pool in ((False, True) if r.pool else (False,))]


def _aff_id(p):
    return "{}{}".format(p[0].id, "-pool" if p[1] else "")


@pytest.mark.parametrize("row,pool", AFF_PARAMS, ids=[_aff_id(p) for p in AFF_PARAMS])
def test_fwd_affine_exact(ops, row, pool):
    z = run_aff(ops, row, pool, "exact")
    if any("lin_sk_fixup_kernel" in k for k in row.kern):      # stream-K: once more without the workspace, the plain kernel
        assert torch.equal(z, run_aff(ops, row, pool, "exact", use_ws=False))


@pytest.mark.parametrize("row,pool", AFF_PARAMS, ids=[_aff_id(p) for p in AFF_PARAMS])
def test_fwd_affine_gaussian(ops, row, pool):
    run_aff(ops, row, pool, "gauss")


def _aff_call(L, ops, shape, prec, pool, pool_s=None):
    """unetk_conv3x3_fwd_affine on zero-filled, full-size operands; returns (rc, trace, outputs)."""
    n, h, w, cin, cout = shape
    from boxsegliver_amd import _abi
    d = _abi.ConvDesc(n, h, w, cin, cout, cin, cout, prec, 1)
    sd = _sd(prec)
    first = not (cin % 16 == 0 and cout % 32 == 0)
    x = torch.zeros((n, h, w, cin), dtype=torch.float32 if first else sd, device="cuda")
    wp = torch.zeros(9 * max(cin, 4) * cout, dtype=torch.float32 if first else sd, device="cuda")
    tab = torch.ones(cout, device="cuda")
    z = torch.full((n, h, w, cout), 3.0, dtype=sd, device="cuda")
    ps = pool_s or cout
    pooled = torch.full((n * ((h + 1) // 2) * ((w + 1) // 2) * ps + 64,), 3.0, dtype=sd, device="cuda")
    rc, names = _trace(ops, lambda: L.unetk_conv3x3_fwd_affine(
        ctypes.byref(d), _p(x), _p(wp), _p(tab), _p(tab), _p(z), _p(pooled) if pool else None, ps if pool else 0, None,
        ctypes.c_size_t(0), _stream()))
    return rc, names, (z, pooled)


AFF_REFUSED = ([(r.id, (r.n, r.h, r.w, r.cin, r.cout), r.prec, False) for r in AFF_ROWS if not r.ok]
               + [(r.id + "-pool", (r.n, r.h, r.w, r.cin, r.cout), r.prec, True) for r in AFF_ROWS if not r.pool]
               + [("odd_pool_%dx%d_%s" % (s[1], s[2], PREC_NAME[s[5]]), s[:5], s[5], True) for s in AFF_ODD_POOL])


@pytest.mark.parametrize("what,shape,prec,pool", AFF_REFUSED, ids=[a[0] for a in AFF_REFUSED])
def test_fwd_affine_refused_shapes(ops, what, shape, prec, pool):
    """unetk_conv3x3_fwd_affine_ok = 0 and UNETK_E_UNSUPPORTED before any launch."""
    L = lib()
    from boxsegliver_amd import _abi
    assert L.unetk_conv3x3_fwd_affine_ok(ctypes.byref(_abi.ConvDesc(*(shape + (shape[3], shape[4], prec, 1)))), int(pool)) == 0
    rc, names, outs = _aff_call(L, ops, shape, prec, pool)
    assert rc == E_UNSUPPORTED and names == [], (what, rc, names)
    assert all(bool((o == 3.0).all()) for o in outs)


@pytest.mark.parametrize("rid,pool_s", [("aff_bs_v3_128", 256 + 4), ("aff_bs_v3_64", 64 + 2)])
def test_persistent_kernel_refuses_a_pool_stride_it_cannot_store(ops, rid, pool_s):
    """The persistent kernel stores a pooled pixel's channels as 16-byte (64-wide tile: 8-byte) units: pool_s % 8 (% 4)."""
    r = AFF_BY_ID[rid]
    rc, names, outs = _aff_call(lib(), ops, (r.n, r.h, r.w, r.cin, r.cout), r.prec, True, pool_s=pool_s)
    assert rc == E_UNSUPPORTED and names == [], (rc, names)
    assert all(bool((o == 3.0).all()) for o in outs)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_tables_reach_every_named_kernel(ops):
    """The union of the asserted traces of the exact tier contains every kernel the two entry points can launch."""
    for r, ps, sliced in NBR_PARAMS:
        if not sliced and (r.id, ps) not in TRACED:
            run_nbr(ops, r, ps, "exact")
    for r, pool in AFF_PARAMS:
        if (r.id, pool) not in TRACED:
            run_aff(ops, r, pool, "exact")
    union = set()
    for names in TRACED.values():
        union |= names
    missing = [k for k in REQUIRED if not any(k in n for n in union)]
    assert not missing, missing
