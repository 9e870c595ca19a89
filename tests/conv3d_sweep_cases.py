"""The extent sweep of the 3-D conv composition (csrc/conv3d.hip), shared by test_conv3d_sweep_host.py (no GPU) and
test_gpu_conv3d_sweep.py: the grid of cases, the two exact input kinds, and a restatement of the dispatch.

conv3d.hip builds every UNet3D convolution out of 2-D kernels and sends the forward, the input gradient and the filter gradient
down one of about a dozen branches chosen by extents, parities and channel counts.  The index arithmetic of those branches
(tap_range, the SAME pads, the space-to-depth and parity classes, Tap / WgRun::lo / hi, the ImgAddr plane strides) is the kind that
breaks at one residue and not the next, so the sweep runs every branch over a dense grid of small and odd extents with inputs
for which fp32 arithmetic is exact in any summation order, and compares bit for bit with float64.

branch(case) restates the predicates of conv3d.hip (the route tests of conv3d_plan, tap_range, wg_runs), conv_igemm_lin.hip
(lin_ok, lin_rows_bound, unetk_conv_lin_gen_ok), conv_igemm.hip (unetk_conv_stride2_ok) and conv_wgrad.hip (the channel rule of
unetk_wgrad_plan at stride 2) with the default switches; decode(case, op, launches) names the branch a traced launch list shows.
The device test asserts that the two agree for every case, so a change of the dispatch cannot quietly move the cases elsewhere.
"""
import collections
import zlib

import torch

DS = (1, 2, 3, 4, 5)
HS = (1, 2, 3, 5, 8, 9)
WS = (1, 2, 3, 5, 6, 7, 12, 13, 16, 17, 31, 32, 33)
SUB_DS = (1, 2, 3)
SUB_HS = (1, 2, 5, 8)
SUB_WS = (1, 2, 6, 13, 16, 17, 33)
# (kd, stride) of UNet3D's layers
FAMILIES = ((1, (1, 1, 1)), (1, (1, 2, 2)), (3, (1, 1, 1)), (3, (1, 2, 2)), (3, (2, 2, 2)))
STRIDE2_FAMILIES = FAMILIES[1], FAMILIES[3], FAMILIES[4]
# (64, 64): the full grid.  (32, 32) reaches the subsample forward and the dilated filter gradient, (64, 128) the 64-pixel-block
# and 128-wide linear variants: the sub-grid.
CHANNELS = ((64, 64), (32, 32), (64, 128))
ITEMS = [(f, c) for f in FAMILIES for c in CHANNELS]
SLICE_EXTRA = 32        # a sliced case: x / dx and y / dy live in buffers 32 channels wider, as a concat half does

# xoff / yoff: channel offset of the view inside the wider buffer; sliced False = dense buffers
Case = collections.namedtuple("Case", "n d h w cin cout kd stride sliced xoff yoff")


def item_id(item):
    (kd, s), (cin, cout) = item
    return "k{}s{}{}{}-{}x{}".format(kd, s[0], s[1], s[2], cin, cout)


def extents(channels):
    full = tuple(channels) == CHANNELS[0]
    return [(d, h, w) for d in (DS if full else SUB_DS) for h in (HS if full else SUB_HS) for w in (WS if full else SUB_WS)]


def cases(family, channels):
    """The cases of one (family, channel pair) item.  Odd positions of the list are the channel-slice cases, and those
    alternate which of the two tensors sits in the upper half of its buffer."""
    kd, stride = family
    cin, cout = channels
    out = []
    for i, (d, h, w) in enumerate(extents(channels)):
        sliced = i % 2 == 1
        xoff = SLICE_EXTRA if sliced and i % 4 == 1 else 0
        yoff = SLICE_EXTRA if sliced and i % 4 == 3 else 0
        out.append(Case(1 + (d + h + w) % 2, d, h, w, cin, cout, kd, tuple(stride), sliced, xoff, yoff))
    return out


def case_id(c):
    return "{}x{}x{}x{} {}->{} k{} s{}{}".format(c.n, c.d, c.h, c.w, c.cin, c.cout, c.kd, "".join(map(str, c.stride)),
                                                 " sliced" if c.sliced else "")


def seed(c, kind):
    return zlib.crc32(repr((kind,) + tuple(c[:8])).encode())


# ------------------------------------------------------------------------------------------------ geometry (conv3d.hip geo3)
def same_pb(n, k, s):
    out = (n + s - 1) // s
    return max((out - 1) * s + k - n, 0) // 2


Geo = collections.namedtuple("Geo", "do ho wo pb_d")


def geo(c):
    sd, shw = c.stride[0], c.stride[1]
    return Geo((c.d + sd - 1) // sd, (c.h + shw - 1) // shw, (c.w + shw - 1) // shw, same_pb(c.d, c.kd, sd))


def out_shape(c):
    g = geo(c)
    return (c.n, g.do, g.ho, g.wo, c.cout)


def tap_range(c, dt):
    """Output planes lo .. hi that depth tap dt reaches: 0 <= do * sd - pb + dt < D (hi < lo: none)."""
    g, sd = geo(c), c.stride[0]
    lo = g.pb_d - dt
    lo = 0 if lo <= 0 else (lo + sd - 1) // sd
    hi = c.d - 1 + g.pb_d - dt
    hi = -1 if hi < 0 else hi // sd
    return lo, min(hi, g.do - 1)


def live_taps(c):
    return [dt for dt in range(c.kd) if tap_range(c, dt)[1] >= tap_range(c, dt)[0]]


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(c, kind):
    """CPU float64 x [N,D,H,W,Cin], w [kd,3,3,Cin,Cout], dy [N,Do,Ho,Wo,Cout]: the two exact kinds of
    tests/test_gpu_conv_paths.py make_inputs carried to 5-D.
      eighths: x integers in [-4, 4], w eighths in [-2, 2] / 8, dy integers in [-2, 2];
      sparse:  ternary, about 1.5 non-zero products per output (density sqrt(1.5 / (9 kd Cin)))."""
    g = torch.Generator().manual_seed(seed(c, kind))
    xs, ws, ys = (c.n, c.d, c.h, c.w, c.cin), (c.kd, 3, 3, c.cin, c.cout), out_shape(c)
    if kind == "eighths":
        x = torch.randint(-4, 5, xs, generator=g).double()
        w = torch.randint(-2, 3, ws, generator=g).double() / 8
        dy = torch.randint(-2, 3, ys, generator=g).double()
        return x, w, dy
    assert kind == "sparse"
    dens = min(1.0, (1.5 / (9.0 * c.kd * c.cin)) ** 0.5)

    def tern(shape):
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double() * (torch.rand(shape, generator=g) < dens).double()
    return tern(xs), tern(ws), tern(ys)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
CK, LIN_BM, LIN_MAXPIX = 16, 128, 416


def lin_rows_bound(h, w, bm=LIN_BM):
    """conv_igemm_lin.hip: padded rows a block of bm linear pixels may touch."""
    if bm % w == 0 and (h * w) % bm == 0:
        return bm // w + 2
    return (bm + w - 1) // w + 1 + 2 + 2 * ((bm + h * w - 1) // (h * w))


def lin_gen_ok(h, w, cin, cout):
    """unetk_conv_lin_gen_ok: the four-class kernel takes an h x w dy plane (cin = dy channels, cout = dx channels)."""
    bm = 64 if cout % 128 == 0 else LIN_BM
    return cin % CK == 0 and cout % 32 == 0 and lin_rows_bound(h, w, bm) * (w + 2) <= LIN_MAXPIX


def lin_ok(n, h, w, cin, cout, spg):
    """lin_ok at the default UNETK_LIN_2D: the linear-pixel kernel takes n planes of h x w in groups of spg."""
    if cin % CK != 0 or cout % 64 != 0 or w >= 32 or spg < 1 or n % spg != 0:
        return False
    gpix = spg * h * w
    lin = (gpix + LIN_BM - 1) // LIN_BM * LIN_BM
    tiled = spg * ((h + 7) // 8) * 8 * ((w + 15) // 16) * 16
    tiled_blocks = (n // spg) * tiled // 64 * (cout // (128 if cout % 128 == 0 else 64))
    starved = cout % 128 == 0 and tiled_blocks <= 256 and gpix % 64 == 0
    if lin * 10 > tiled * 9 and not starved:
        return False
    rows = (LIN_BM + w - 1) // w + 1 + 2 + 2 * ((LIN_BM + h * w - 1) // (h * w))
    return rows * (w + 2) <= LIN_MAXPIX


def stride2_ok(cin, cout):
    return cin % CK == 0 and cout % 64 == 0


def s2lin_ok(c):
    """conv3d_plan's test for FWD_S2D (at the default UNETK_S2LIN)."""
    g = geo(c)
    if c.stride[1] != 2 or c.h % 2 or c.w % 2 or c.cin % 16:
        return False
    if c.stride[0] == 2 and (c.d % 2 or c.kd != 3):
        return False
    return lin_ok(c.n * g.do, g.ho, g.wo, c.cin, c.cout, g.do)


def wgrad_native(c):
    """unetk_wgrad_plan at stride 2 takes the channels (fp32)."""
    return c.stride[1] == 2 and c.cin % 32 == 0 and c.cout % 64 == 0


F_TAP_TILED, F_TAP_LIN, F_FUSED_LIN = "fwd per-tap tiled", "fwd per-tap linear", "fwd fused-tap linear"
F_S2D, F_S2_KD1, F_S2_KD3, F_SUB = "fwd s2d + grouped taps", "fwd native stride-2 kd=1", "fwd native stride-2 fused kd=3", \
    "fwd stride-1 + subsample"
D_TAP, D_FUSED_LIN = "dgrad per-tap", "dgrad fused-tap linear"
D_GEN_TAP, D_GEN_FUSED, D_GEN_DPAR, D_DILATED = "dgrad four-class per tap", "dgrad four-class fused depth", \
    "dgrad four-class dpar", "dgrad dilated fallback"
W_S1_TAP, W_S1_FUSED = "wgrad stride-1 per tap", "wgrad stride-1 fused kd"
W_S2_TAP, W_S2_FUSED = "wgrad native stride-2 per tap", "wgrad native stride-2 fused kd"
W_DIL_KD1, W_DIL_TAPS = "wgrad dilated kd=1", "wgrad dilated per tap kd=3"
# Every branch of the composition.  (A dilated filter gradient with fused depth taps does not exist: wg_runs fuses the taps only
# of a stride-1 or natively strided launch.)
BRANCHES = (F_TAP_TILED, F_TAP_LIN, F_FUSED_LIN, F_S2D, F_S2_KD1, F_S2_KD3, F_SUB,
            D_TAP, D_FUSED_LIN, D_GEN_TAP, D_GEN_FUSED, D_GEN_DPAR, D_DILATED,
            W_S1_TAP, W_S1_FUSED, W_S2_TAP, W_S2_FUSED, W_DIL_KD1, W_DIL_TAPS)


def _full_tap(c):
    """The depth tap the forward launches last (conv3d.hip Conv3dPlan::tap: the first tap that covers every output plane)."""
    g = geo(c)
    return next(dt for dt in range(c.kd) if tap_range(c, dt) == (0, g.do - 1))


def branch(c):
    """(forward, input-gradient, filter-gradient) branch of a case.  Where the launches of one op could differ per depth tap
    (each tap's launch is planned at its own plane count) the op is named by its last launch, as decode() reads it."""
    g = geo(c)
    sd, shw = c.stride[0], c.stride[1]
    # ---- forward
    if c.kd == 3 and sd == 1 and shw == 1 and lin_ok(c.n * c.d, c.h, c.w, c.cin, c.cout, c.d):
        f = F_FUSED_LIN
    elif s2lin_ok(c):
        f = F_S2D
    elif shw == 2 and stride2_ok(c.cin, c.cout):
        f = F_S2_KD3 if c.kd == 3 else F_S2_KD1
    elif shw == 2:
        f = F_SUB
    else:
        lo, hi = tap_range(c, _full_tap(c))
        f = F_TAP_LIN if lin_ok(c.n * (hi - lo + 1), c.h, c.w, c.cin, c.cout, hi - lo + 1) else F_TAP_TILED
    # ---- input gradient (the conv of dy with Cin and Cout swapped)
    if shw == 2 and lin_gen_ok(g.ho, g.wo, c.cout, c.cin):
        if c.kd == 3 and sd == 2 and c.d % 2 == 0 and g.pb_d == 0:
            dg = D_GEN_DPAR
        elif c.kd == 3 and sd == 1:
            dg = D_GEN_FUSED
        else:
            dg = D_GEN_TAP
    elif shw == 2:
        dg = D_DILATED
    elif c.kd == 3 and sd == 1 and lin_ok(c.n * c.d, c.h, c.w, c.cout, c.cin, c.d):
        dg = D_FUSED_LIN
    else:
        dg = D_TAP
    # ---- filter gradient
    if shw == 1:
        wg = W_S1_FUSED if c.kd == 3 else W_S1_TAP
    elif wgrad_native(c):
        wg = W_S2_FUSED if c.kd == 3 else W_S2_TAP
    else:
        wg = W_DIL_TAPS if c.kd == 3 else W_DIL_KD1
    return f, dg, wg


# ------------------------------------------------------------------------------------------------ the launch trace, decoded
LIN, IGEMM, WGK = "conv3x3_igemm_lin_kernel", "conv3x3_igemm_kernel", "conv3x3_wgrad_kernel"


def _targs(name):
    return name[name.index("<") + 1:name.rindex(">")].split(",")


def _lin_flags(name):
    """GEN, FUSED (the four classes in one block), SK, ACC, GRP of a conv3x3_igemm_lin_kernel instantiation."""
    a = _targs(name)
    return {k: a[i] == "true" for k, i in (("GEN", 4), ("FUSED", 5), ("SK", 6), ("ACC", 7), ("GRP", 8))}


def _is_acc(name):
    if name.startswith(LIN):
        return _lin_flags(name)["ACC"]
    return name.startswith(IGEMM) and _targs(name)[6] == "1"


def decode(c, op, launches):
    """The branch a launch list (names as tests/test_gpu_ops3d.py _trace writes them: no blanks, no argument list) shows for
    op "fwd" / "dgrad" / "wgrad" of case c, or a string starting with "?" that says what does not fit any branch.  The trace
    holds kernels only (a memset is not a launch), so an accumulating sequence is known by the ACC flag / MODE 1 of its
    kernels and, over a channel slice, by zero_slice_kernel."""
    convs = [n for n in launches if n.startswith(LIN) or n.startswith(IGEMM)]
    taps = len(live_taps(c))
    acc = [_is_acc(n) for n in convs]
    multi = c.kd > 1 or c.stride[0] > 1            # the per-tap sequences of this op accumulate into a zeroed output

    def stride1(n):                                # a plain stride-1 launch of either kernel family
        return (n.startswith(LIN) and not _lin_flags(n)["GEN"] and not _lin_flags(n)["GRP"]) or \
            (n.startswith(IGEMM) and _targs(n)[4] == "1")

    def per_tap(ok_names, label, accumulates):
        if len(convs) != taps or not all(ok_names(n) for n in convs) or (accumulates is not None and any(a != accumulates for a in acc)):
            return "?{}: {} launches for {} taps, accumulate {}".format(label, len(convs), taps, acc)
        return label

    if op == "fwd":
        if launches and launches[0] == "s2d_kernel":
            ok = len(convs) == 1 and convs[0].startswith(LIN) and _lin_flags(convs[0])["GRP"] and not acc[0]
            return F_S2D if ok else "?s2d without one grouped-tap launch"
        if launches and launches[-1] == "subsample2_stats_kernel":
            return per_tap(stride1, F_SUB, c.kd > 1)
        if convs and all(n.startswith(IGEMM) and _targs(n)[4] == "2" for n in convs):
            if len(convs) != 1 or acc[0]:
                return "?native stride-2 forward in {} launches".format(len(convs))
            return F_S2_KD3 if c.kd == 3 else F_S2_KD1
        if not convs or c.stride[1] != 1:
            return "?no forward branch"
        last = convs[-1]
        if c.kd == 3 and len(convs) == 1 and last.startswith(LIN) and not acc[0]:
            return F_FUSED_LIN
        return per_tap(stride1, F_TAP_LIN if last.startswith(LIN) else F_TAP_TILED, c.kd > 1)
    if op == "dgrad":
        if launches and launches[0] == "dilate2_kernel":
            return per_tap(stride1, D_DILATED, multi)
        if convs and all(n.startswith(LIN) and _lin_flags(n)["GEN"] for n in convs):
            if not all(_lin_flags(n)["FUSED"] for n in convs):
                return "?four-class launch per parity class"
            # (this variant accumulates by a run-time flag, not a template one: its sequences are known by their length, and the
            # one launch of an odd depth-stride-2 layer with a single live tap by the case)
            if c.kd == 3 and len(convs) == 1 and (c.stride[0] == 1 or c.d % 2 == 0):
                return D_GEN_DPAR if c.stride[0] == 2 else D_GEN_FUSED
            return per_tap(lambda n: True, D_GEN_TAP, None)
        if not convs or c.stride[1] != 1:
            return "?no input-gradient branch"
        if c.kd == 3 and len(convs) == 1 and convs[0].startswith(LIN) and not acc[0]:
            return D_FUSED_LIN
        return per_tap(stride1, D_TAP, multi)
    assert op == "wgrad"
    wg = [n for n in launches if n.startswith(WGK)]
    dil = bool(launches) and launches[0] == "dilate2_kernel"
    native = [_targs(n)[6] == "2" for n in wg]
    if not wg or any(native) != all(native) or (dil and any(native)):
        return "?no filter-gradient branch"
    if dil:
        if len(wg) != taps:
            return "?dilated filter gradient: {} launches for {} taps".format(len(wg), taps)
        return W_DIL_TAPS if c.kd == 3 else W_DIL_KD1
    if len(wg) != 1:
        return "?{} undilated filter-gradient launches".format(len(wg))
    if all(native):
        return W_S2_FUSED if c.kd == 3 else W_S2_TAP
    if c.stride[1] != 1:
        return "?stride-1 filter gradient of a strided conv without dilate2_kernel"
    return W_S1_FUSED if c.kd == 3 else W_S1_TAP
