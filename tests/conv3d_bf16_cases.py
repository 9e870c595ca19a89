"""Case table, inputs and float64 reference shared by tests/test_gpu_conv3d_bf16_paths.py (on the device) and
tests/test_conv3d_bf16_paths_host.py (no GPU).  Nothing here touches the device unless a caller asks for dev="cuda".

Every row was written out by hand from the predicates of csrc/conv_igemm_bf16.hip (pick_bf16, unetk_conv_plan_bf16,
unetk_conv_launch_bf16), csrc/conv_wgrad.hip (unetk_wgrad_plan at UNETK_BF16 with kd, unetk_wgrad_run, unetk_launch_slab_reduce) and
csrc/conv3d.hip (unetk_conv3d_{fwd,dgrad,wgrad}_bf16: the forward picks its tile from (N D, H, W, Cin, Cout), the input gradient
from the same with Cin and Cout swapped).  pick_bf16 / wg_splits below restate those predicates; the host test holds every row
against them, so that a row and the restatement can only be wrong together, and the device test holds every row against the
library's launch trace.
"""
import collections

import torch

from oracle import tf_ops

BFK = "conv3x3_igemm_bf16_kernel<"
# tile configurations of pick_bf16: id -> (template head WM,WN,TM,TN, tile height in pixels; every tile is 16 pixels wide)
CFG = {0: ("4,2,4,2", 32), 1: ("2,2,2,2", 8), 2: ("4,1,2,2", 16), 3: ("4,1,1,2", 8), 4: ("4,1,2,1", 16)}
TW = 16
WG_TH = 8           # the filter gradient's plain tile: 8 x 16 pixels


def bf(cfg, ft):
    """Trace name of tile configuration cfg; ft = the fused-depth-tap instantiation (kd = 3)."""
    return "{}{},false,false,{}>".format(BFK, CFG[cfg][0], "true" if ft else "false")


def wg(cit, cot):
    return "conv3x3_wgrad_kernel<{},{},true,8,16,false,1,1>".format(cit, cot)


def red(k):
    return "slab_reduce_kernel<{}>".format(k)


Case = collections.namedtuple("Case", "id n d h w cin cout kd xpad ypad fwd rows tiles dgrad wgrad splits big")


def _c(id, shape, fwd, rows, tiles, dgrad, wgrad, splits, xpad=0, ypad=0, big=False):
    n, d, h, w, cin, cout, kd = shape
    return Case(id, n, d, h, w, cin, cout, kd, xpad, ypad, fwd, rows, tiles, dgrad, wgrad, splits, big)


# id, (N, D, H, W, Cin, Cout, kd),
#   forward kernel, its statistic rows, (tile height, tiles_h, tiles_w) of the forward,
#   input-gradient kernel,
#   filter-gradient launches in order (no reducer: one split, dw written in place), the plan's splits S
# xpad / ypad: x and dx (dy and y) are channel slices of buffers xpad (ypad) channels wider
# big: the float64 reference runs on the device
CASES = [
    # ---- fused depth taps (kd = 3)
    # forward 512 x 128 with exactly 200 blocks (10 planes x 2 x 10 tiles x 1): second tile row one pixel high, last column 6 wide
    _c("ft_tall_fwd", (2, 5, 33, 150, 32, 128, 3),
       bf(0, True), 200, (32, 2, 10), bf(4, True), [wg(32, 64), red(4)], 42, ypad=4, big=True),
    # the same tile as an input gradient (Cin = 128 is its output width); forward 256 x 64
    _c("ft_tall_dgrad", (2, 5, 33, 150, 128, 64, 3),
       bf(2, True), 300, (16, 3, 10), bf(0, True), [wg(64, 64), red(4)], 42, xpad=4, big=True),
    # a plane smaller than one tile both ways, 128 x 128 forward, 128 x 64 input gradient
    _c("ft_128_small", (2, 3, 7, 13, 64, 128, 3),
       bf(1, True), 6, (8, 1, 1), bf(3, True), [wg(64, 64), red(1)], 6, xpad=8),
    # D = 2: every plane has one depth tap without an input plane; 2 x 2 partial tiles of 256 x 64
    _c("ft_256x64_d2", (1, 2, 19, 21, 32, 64, 3),
       bf(2, True), 8, (16, 2, 2), bf(4, True), [wg(32, 64), red(4)], 12, ypad=8),
    # 256 x 64 as an input gradient; two samples of two planes
    _c("ft_256x64_dgrad", (2, 2, 13, 17, 64, 32, 3),
       bf(4, True), 8, (16, 1, 2), bf(2, True), [wg(64, 32), red(4)], 16, xpad=4, ypad=4),
    # D = 1, one filter-gradient tile: one split, dw[0] and dw[2] written as zeros straight into the output
    _c("ft_d1_single", (1, 1, 8, 16, 64, 64, 3),
       bf(3, True), 1, (8, 1, 1), bf(3, True), [wg(64, 64)], 1),
    # three one-plane samples side by side in memory
    _c("ft_n3_d1", (3, 1, 5, 40, 64, 32, 3),
       bf(4, True), 9, (16, 1, 3), bf(3, True), [wg(64, 32), red(4)], 9, ypad=4),
    _c("ft_32x32", (2, 4, 16, 32, 32, 32, 3),
       bf(4, True), 16, (16, 1, 2), bf(4, True), [wg(32, 32), red(4)], 32, xpad=4),
    # bridge/conv2: 30 (tap, chunk) steps, K = 8640
    _c("ft_bridge", (1, 3, 6, 6, 320, 320, 3),
       bf(3, True), 3, (8, 1, 1), bf(3, True), [wg(64, 64), red(1)], 3),
    # conv_d3/conv1: the concat read, K = 13824; 128 x 128 both ways
    _c("ft_concat", (1, 2, 12, 12, 512, 256, 3),
       bf(1, True), 4, (8, 2, 1), bf(1, True), [wg(64, 64), red(1)], 2, xpad=64),
    # ---- plain planes (kd = 1) through the 3-D entry points: the ImgAddr plane addressing
    _c("k1_tall", (1, 10, 33, 150, 32, 128, 1),
       bf(0, False), 200, (32, 2, 10), bf(4, False), [wg(32, 64), red(16)], 125, xpad=4, big=True),
    _c("k1_96", (2, 3, 9, 17, 96, 96, 1),
       bf(4, False), 12, (16, 1, 2), bf(4, False), [wg(32, 32), red(4)], 24, xpad=8),
    _c("k1_128", (2, 2, 10, 20, 64, 128, 1),
       bf(1, False), 16, (8, 2, 2), bf(3, False), [wg(64, 64), red(4)], 16, ypad=4),
    _c("k1_64", (3, 1, 13, 18, 64, 64, 1),
       bf(2, False), 6, (16, 1, 2), bf(2, False), [wg(64, 64), red(4)], 12, ypad=4),
    _c("k1_64x32", (1, 3, 5, 19, 64, 32, 1),
       bf(4, False), 6, (16, 1, 2), bf(3, False), [wg(64, 32), red(1)], 6),
]
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------ the predicates, restated
def _cd(a, b):
    return -(-a // b)


def pick_bf16(h, cin, cout, n, w):
    """csrc/conv_igemm_bf16.hip pick_bf16: the tile configuration id (-1: refused)."""
    if cin % 32 != 0 or cout % 32 != 0:
        return -1
    if cout % 128 == 0:
        if h < 24 or n * _cd(h, 32) * _cd(w, TW) * (cout // 128) < 200:
            return 1
        return 0
    if cout % 64 == 0:
        return 2 if h >= 12 else 3
    return 4


def wg_splits(n, h, w, cin, cout, kd):
    """csrc/conv_wgrad.hip unetk_wgrad_plan at UNETK_BF16 (plain tiles, unetk_split): (cit, cot, splits S)."""
    total = n * _cd(h, WG_TH) * _cd(w, TW)
    cit, cot = (64 if cin % 64 == 0 else 32), (64 if cout % 64 == 0 else 32)
    panels = (cin // cit) * (cout // cot) * (kd if kd > 1 else 1)
    s = 1 if panels >= 512 else 512 // panels
    if total // s < 16 and panels <= 256:
        s = 256 // panels
    s = max(1, min(s, total))
    per = _cd(total, s)
    return cit, cot, _cd(total, per)


def reducer(s):
    """unetk_launch_slab_reduce: the reducer a plan of S splits launches (None: S == 1, in place)."""
    return None if s == 1 else red(16 if s >= 64 else 4 if s >= 8 else 1)


# ------------------------------------------------------------------------------------------------ inputs and reference
KINDS = ("eighths", "sparse", "gauss")


def _seed(case, kind):
    return 9100 + sum(ord(ch) for ch in case.id) + KINDS.index(kind)


def make_inputs(case, kind):
    """CPU float32 x [N,D,H,W,Cin], w [kd,3,3,Cin,Cout], dy [N,D,H,W,Cout] and the unit (lsb) of y (None: Gaussian)."""
    g = torch.Generator().manual_seed(_seed(case, kind))
    xs = (case.n, case.d, case.h, case.w, case.cin)
    ws = (case.kd, 3, 3, case.cin, case.cout)
    ys = (case.n, case.d, case.h, case.w, case.cout)
    if kind == "eighths":
        x = torch.randint(-4, 5, xs, generator=g).float()
        w = torch.randint(-2, 3, ws, generator=g).float() / 8
        dy = torch.randint(-2, 3, ys, generator=g).float()
        return x, w, dy, 0.125
    if kind == "sparse":
        # about 1.5 non-zero products per output of an interior plane: max |y| <= 15 with room to spare (asserted by the callers)
        dens = min(1.0, (1.5 / (9.0 * case.kd * case.cin)) ** 0.5)

        def tern(shape):
            return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (torch.rand(shape, generator=g) < dens).float()
        return tern(xs), tern(ws), tern(ys), 1.0
    assert kind == "gauss"
    x = torch.randn(xs, generator=g)
    w = torch.randn(ws, generator=g) / (9 * case.kd * case.cin) ** 0.5
    dy = torch.randn(ys, generator=g)
    return x, w, dy, None


def conv_grads(x64, w64, dy64, conv=tf_ops.conv_nd_same):
    """(y, dx, dw) of `conv` in the dtype of its arguments."""
    xr, wr = x64.detach().requires_grad_(True), w64.detach().requires_grad_(True)
    y = conv(xr, wr)
    dx, dw = torch.autograd.grad(y, (xr, wr), dy64)
    return y.detach(), dx, dw


_REFS = {}


def reference(case, kind, dev="cpu"):
    """float64 (y, dx, dw) of the row's exact inputs and max(conv(|x|, |w|)); computed once per (row, kind, device)."""
    key = (case.id, kind, dev)
    if key not in _REFS:
        assert kind in ("eighths", "sparse")
        x, w, dy, _ = make_inputs(case, kind)
        x64, w64, dy64 = x.to(dev).double(), w.to(dev).double(), dy.to(dev).double()
        y, dx, dw = conv_grads(x64, w64, dy64)
        with torch.no_grad():
            amax = tf_ops.conv_nd_same(x64.abs(), w64.abs()).max().item()
        _REFS[key] = (y, dx, dw, amax)
    return _REFS[key]


def exact_bounds(case, kind, x, w, dy, lsb, y64, amax):
    """The bounds that keep a row's fp32 arithmetic exact in any summation order, from its own inputs."""
    assert amax / lsb < 2 ** 24, (case.id, amax)                                  # y: multiples of lsb below 2^24 lsb
    assert 8 * case.n * case.d * case.h * case.w < 2 ** 24, case.id              # dw: |x dy| <= 8, one term per voxel and tap
    assert float(dy.abs().max()) * float(w.abs().max()) * 9 * case.kd * case.cout / lsb < 2 ** 24    # dx, worst case
    if kind == "sparse":
        assert float(y64.abs().max()) <= 15, (case.id, float(y64.abs().max()))


def tile_stats(y64, case):
    """float64 (sum y, sum y^2) per statistic row [rows, Cout]: row (i tiles_h + th_i) tiles_w + tw_i is the th x 16 tile
    (th_i, tw_i) of plane i."""
    th, tiles_h, tiles_w = case.tiles
    planes = y64.reshape(case.n * case.d, case.h, case.w, case.cout)
    pad = torch.zeros((planes.shape[0], tiles_h * th, tiles_w * TW, case.cout), dtype=planes.dtype, device=planes.device)
    pad[:, :case.h, :case.w] = planes
    t = pad.reshape(planes.shape[0], tiles_h, th, tiles_w, TW, case.cout)
    return t.sum((2, 4)).reshape(-1, case.cout), (t * t).sum((2, 4)).reshape(-1, case.cout)
