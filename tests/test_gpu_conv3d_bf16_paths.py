"""The bf16 3-D convolution entry points (unetk_conv3d_fwd_bf16 / _dgrad_bf16 / _wgrad_bf16: --compute_dtype bf16c, thirteen of
UNet3D's eighteen convs) on every dispatch path, with inputs for which the arithmetic is exact in any summation order.

What is pinned.  Forward and input gradient launch conv3x3_igemm_bf16_kernel<WM,WN,TM,TN,false,false,FT>: FT = true contracts
the three depth taps of a (3,3,3) conv in one launch and skips, per block, the taps whose input plane lies outside the sample;
FT = false (kd = 1) is the plain 2-D instance run over the N D planes through the ImgAddr plane addressing.  The filter gradient
launches the bf16 conv3x3_wgrad_kernel<CIT,COT,true,...> with WgParams::kd = kd, one block per (split, depth tap, panel), and
reduces the splits' slabs in fixed order -- or, for one split, writes dw in place.  The table (tests/conv3d_bf16_cases.py)
reaches all five tile shapes with FT on (each as a forward with statistics and as an input gradient) and off, all four
filter-gradient panel shapes with kd = 3 and kd = 1, the single-split in-place path with kd = 3, and the depth edges: D = 1
(taps 0 and 2 have no input plane: the FT kernel runs the middle tap only, the filter gradient writes zeros into dw[0] and
dw[2]), D = 1 and D = 2 with N > 1 (the neighbour plane in memory is another sample's, real data rather than a zero page),
planes with partial tiles both ways and planes smaller than a tile.

How the table was derived.  Every row names its forward kernel, statistic rows and tile geometry, its input-gradient kernel
and its filter-gradient launches, written out by hand from pick_bf16, unetk_conv_plan_bf16, unetk_wgrad_plan (UNETK_BF16, kd)
and unetk_wgrad_run; tests/test_conv3d_bf16_paths_host.py holds the rows against a restatement of those predicates without a
device.  Here the library's launch trace of every call must equal the row exactly, so a row that lands elsewhere after a
dispatch change fails instead of quietly testing something else.

Tiers.  "eighths": x integers in [-4, 4], w eighths in [-2/8, 2/8], dy integers in [-2, 2] -- bf16 holds them exactly, every
partial sum is a multiple of 1/8 (1 for dw) far below 2^24 units, so y, dx and dw equal the float64 convolution
(oracle.tf_ops.conv_nd_same) bit for bit; each row asserts the bounds of that regime from its own inputs.  "sparse": x, w in
{-1, 0, 1} with max |y| <= 15, so every statistic partial is exact too and each statistic row is compared with the float64
sums over exactly its tile.  Gaussian: the bounds of test_gpu_unet3d_bf16c.py unchanged -- 2e-5 of sum |a b| for y, dx, dw
against float64 on the bf16-rounded operands, statistics at 1e-5, and the exact-fp32 path differing by more than 3e-5 and more
than five times the measured error (the bf16 pipe really ran).  No other tolerance appears.

Every call goes through the C ABI with guarded buffers (tests/guardbuf.py): x / dx and dy / y are channel slices of wider
buffers on the rows with xpad / ypad, the workspace is exactly unetk_conv3d_ws_bytes_bf16, neighbour channels and guards must
stay bit-equal, no sentinel may remain inside an output, inputs and packed filters stay unchanged, and a short or missing
workspace is refused.

Limits.  ConvParams::accumulate and the inference epilogue (asc) are refused by the FT dispatch (UNETK_E_UNSUPPORTED in
unetk_conv_launch_bf16) and no 3-D entry point sets them; strided 3-D convs, kd = 3 with depth stride 2 and channel counts that
are no multiple of 32 are refused by the entry points (test_refusals) and run exact fp32 in the net.  The live-channel masks of
the descriptor are not used in this mode.  Small rows take the float64 reference on the CPU, rows marked big on the device.
"""
import ctypes

import pytest
import torch

import conv3d_bf16_cases as T
import guardbuf
from oracle import tf_ops

pytestmark = pytest.mark.gpu

E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
CASES = T.CASES
IDS = [c.id for c in CASES]

TRACED = {}     # row id -> {"fwd": [...], "dgrad": [...], "wgrad": [...]}: the launches of the row's three calls


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


def _p(t):
    if t is None:
        return None
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.ptr() if hasattr(t, "ptr") else t.data_ptr())


def _stream(s=None):
    return ctypes.c_void_p((s or torch.cuda.current_stream()).cuda_stream)


def _norm(name):
    name = name.replace(" ", "").replace("(anonymousnamespace)::", "").split("(")[0]
    return name[4:] if name.startswith("void") else name


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return out, [_norm(n) for n in ops.profile_read()[1]]         # every launch, in order


def _coff(pad):
    """Channel offset of a slice in a buffer `pad` channels wider: a multiple of 4 (16-byte alignment), neighbours on both
    sides from 8 channels on."""
    return pad if pad < 8 else pad // 8 * 4


OWN = object()        # "the row's own guarded workspace"


class Row(object):
    """The guarded device buffers of one row and its three calls."""

    def __init__(self, ops, case, x, w, dy):
        from boxsegliver_amd import _abi
        c = self.case = case
        self.xs, self.ys = c.cin + c.xpad, c.cout + c.ypad
        xo, yo = _coff(c.xpad), _coff(c.ypad)
        xshape, yshape = (c.n, c.d, c.h, c.w, c.cin), (c.n, c.d, c.h, c.w, c.cout)
        self.d = ops.conv3d_desc(xshape, c.cout, c.kd, (1, 1, 1), x_stride=self.xs, y_stride=self.ys)
        assert ops.conv3d_bf16_ok(self.d)
        self.nws = lib().unetk_conv3d_ws_bytes_bf16(ctypes.byref(self.d))
        self.rows = lib().unetk_conv3d_stat_rows_bf16(ctypes.byref(self.d))
        assert self.nws > 0 and self.rows == c.rows, (c.id, self.nws, self.rows)
        self.w = w.cuda()
        wp_f, wp_d = ops.conv3d_pack(self.w, precision=_abi.BF16)
        assert wp_f.dtype == torch.bfloat16 and wp_f.numel() == c.kd * 9 * c.cin * c.cout
        self.gx = guardbuf.guarded_input(x.cuda(), self.xs, xo)
        self.gdy = guardbuf.guarded_input(dy.cuda(), self.ys, yo)
        self.gwf = guardbuf.guarded_input(wp_f.reshape(-1, 8))
        self.gwd = guardbuf.guarded_input(wp_d.reshape(-1, 8))
        self.gy = guardbuf.guarded(yshape, torch.float32, self.ys, yo)
        self.gs = guardbuf.guarded((2, self.rows, c.cout))
        self.gdx = guardbuf.guarded(xshape, torch.float32, self.xs, xo)
        self.gdw = guardbuf.guarded((c.kd, 3, 3, c.cin, c.cout))
        self.ws = guardbuf.GuardedWorkspace(self.nws)

    def fwd(self, ws=OWN, nb=None, st=None):
        return lib().unetk_conv3d_fwd_bf16(ctypes.byref(self.d), _p(self.gx), _p(self.gwf), _p(self.gy), _p(self.gs),
                                           _p(self.ws.ptr() if ws is OWN else ws), self.nws if nb is None else nb, _stream(st))

    def dgrad(self, ws=OWN, nb=None, st=None):
        return lib().unetk_conv3d_dgrad_bf16(ctypes.byref(self.d), _p(self.gdy), _p(self.gwd), _p(self.gdx),
                                             _p(self.ws.ptr() if ws is OWN else ws), self.nws if nb is None else nb, _stream(st))

    def wgrad(self, ws=OWN, nb=None, st=None):
        return lib().unetk_conv3d_wgrad_bf16(ctypes.byref(self.d), _p(self.gx), _p(self.gdy), _p(self.gdw),
                                             _p(self.ws.ptr() if ws is OWN else ws), self.nws if nb is None else nb, _stream(st))

    def edges(self, tag, outs, ins):
        for name, o in outs.items():
            assert o.changed_outside() == 0, "{}: {} elements outside `{}` changed".format(tag, o.changed_outside(), name)
            assert o.unwritten() == 0, "{}: {} elements of `{}` never written".format(tag, o.unwritten(), name)
        for name, i in ins.items():
            assert i.changed_anywhere() == 0, "{}: read-only input `{}` changed".format(tag, name)
        assert self.ws.guard_intact(), "{}: the workspace was used beyond its {} bytes".format(tag, self.nws)

    def run(self, ops, tag):
        """The three calls, each with its launch trace held against the row and its buffer edges checked; returns clones of
        y, the statistic partials, dx and dw."""
        c = self.case
        names = {}
        rc, names["fwd"] = _trace(ops, self.fwd)
        assert rc == 0, (tag, "forward", rc)
        assert names["fwd"] == [c.fwd], "{} forward: traced {} expected {}".format(tag, names["fwd"], [c.fwd])
        self.edges(tag + " forward", {"y": self.gy, "stats": self.gs}, {"x": self.gx, "w": self.gwf})
        rc, names["dgrad"] = _trace(ops, self.dgrad)
        assert rc == 0, (tag, "input gradient", rc)
        assert names["dgrad"] == [c.dgrad], "{} input gradient: traced {} expected {}".format(tag, names["dgrad"], [c.dgrad])
        self.edges(tag + " input gradient", {"dx": self.gdx}, {"dy": self.gdy, "w": self.gwd})
        rc, names["wgrad"] = _trace(ops, self.wgrad)
        assert rc == 0, (tag, "filter gradient", rc)
        assert names["wgrad"] == list(c.wgrad), "{} filter gradient: traced {} expected {}".format(tag, names["wgrad"], c.wgrad)
        self.edges(tag + " filter gradient", {"dw": self.gdw}, {"x": self.gx, "dy": self.gdy})
        TRACED[c.id] = names
        return self.gy.view.clone(), self.gs.view.clone(), self.gdx.view.clone(), self.gdw.view.clone()

    def dw_again_and_on_a_side_stream(self, ops, dw, tag):
        """dw is bit-reproducible call to call, and on a side stream with a workspace of its own."""
        self.gdw.reset()
        assert self.wgrad() == 0
        torch.cuda.synchronize()
        assert torch.equal(self.gdw.view, dw), tag + " dw twice"
        self.gdw.reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            own = ops._Workspace().get(self.nws, self.gdw.view.device)
            rc = self.wgrad(ws=own, st=side)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(self.gdw.view, dw), tag + " dw on a side stream"
        assert self.gdw.changed_outside() == 0 and self.gdw.unwritten() == 0

    def workspace_refusals(self, ops, tag):
        """A short workspace is UNETK_E_WORKSPACE, a missing one UNETK_E_BADARG; neither launches or writes anything."""
        outs = (self.gy, self.gs, self.gdx, self.gdw)
        for o in outs:
            o.reset()
        for what, call in (("forward", self.fwd), ("input gradient", self.dgrad), ("filter gradient", self.wgrad)):
            rc, names = _trace(ops, lambda: call(nb=self.nws - 16))
            assert rc == E_WORKSPACE and names == [], (tag, what, "short", rc, names)
            rc, names = _trace(ops, lambda: call(ws=None))
            assert rc == E_BADARG and names == [], (tag, what, "NULL", rc, names)
        for o in outs:
            assert o.changed_anywhere() == 0, tag


def run_exact(ops, case, kind):
    assert kind in ("eighths", "sparse")
    tag = "{} {}".format(case.id, kind)
    x, w, dy, lsb = T.make_inputs(case, kind)
    y64, dx64, dw64, amax = T.reference(case, kind, "cuda" if case.big else "cpu")
    T.exact_bounds(case, kind, x, w, dy, lsb, y64, amax)
    y64, dx64, dw64 = y64.cuda(), dx64.cuda(), dw64.cuda()
    r = Row(ops, case, x, w, dy)
    y, stats, dx, dw = r.run(ops, tag)
    assert torch.equal(y.double(), y64), tag + " y"
    assert torch.equal(dx.double(), dx64), tag + " dx"
    assert torch.equal(dw.double(), dw64), tag + " dw"
    if case.kd == 3 and case.d == 1:          # the taps without an input plane: zeros, written (no sentinel left: edges above)
        assert float(dw[0].abs().max()) == 0.0 and float(dw[2].abs().max()) == 0.0, tag
    # ---- statistic partials, row by row: row (i tiles_h + th_i) tiles_w + tw_i holds the sums over tile (th_i, tw_i) of plane i
    assert tuple(stats.shape) == (2, case.rows, case.cout) and case.rows % case.n == 0
    s1, s2 = T.tile_stats(y64, case)
    pix = case.tiles[0] * T.TW
    ymax = float(y64.abs().max())
    s = stats.double()
    if kind == "sparse":
        assert ymax <= 15 and pix * ymax * ymax < 2 ** 24
    if pix * ymax / lsb < 2 ** 24:            # every partial sum of y is exact
        assert torch.equal(s[0], s1), tag + " sum y per tile"
        per = s[0].reshape(case.n, case.rows // case.n, case.cout).sum(1)
        assert torch.equal(per, y64.sum((1, 2, 3))), tag + " sum y per sample"
    if pix * ymax * ymax / (lsb * lsb) < 2 ** 24:
        assert torch.equal(s[1], s2), tag + " sum y^2 per tile"
        per = s[1].reshape(case.n, case.rows // case.n, case.cout).sum(1)
        assert torch.equal(per, (y64 * y64).sum((1, 2, 3))), tag + " sum y^2 per sample"
    r.dw_again_and_on_a_side_stream(ops, dw, tag)
    r.workspace_refusals(ops, tag)


@pytest.mark.parametrize("kind", ["eighths", "sparse"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv3d_bf16_paths_exact(ops, case, kind):
    run_exact(ops, case, kind)


def _r(t):
    return tf_ops.bf16_round(t)


def _ref(x, w, dy):
    """float64 on bf16-rounded operands and the magnitudes sum |a b| the accumulation-order noise scales with
    (test_gpu_unet3d_bf16c.py)."""
    y, dx, dw = T.conv_grads(_r(x), _r(w), _r(dy))
    ya, dxa, dwa = T.conv_grads(_r(x).abs(), _r(w).abs(), _r(dy).abs())
    return y, dx, dw, ya, dxa, dwa


def _err(got, ref, mag):
    return ((got.double() - ref).abs() / mag.clamp_min(1e-30)).max().item()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv3d_bf16_paths_gaussian(ops, case):
    """Operands bf16 does not hold exactly, with the bounds of test_gpu_unet3d_bf16c.py unchanged."""
    n, cout = case.n, case.cout
    x, w, dy, _ = T.make_inputs(case, "gauss")
    r = Row(ops, case, x, w, dy)
    xg, dyg = r.gx.view, dy.cuda()
    y_ref, dx_ref, dw_ref, y_mag, dx_mag, dw_mag = _ref(xg.double(), r.w.double(), dyg.double())
    y, stats, dx, dw = r.run(ops, case.id + " gauss")
    ey, edx, edw = _err(y, y_ref, y_mag), _err(dx, dx_ref, dx_mag), _err(dw, dw_ref, dw_mag)
    print("gauss", case.id, "y", ey, "dx", edx, "dw", edw)

    # statistic partials: each sample's rows contiguous, fp32 sums of the fp32 accumulators
    assert case.rows % n == 0
    per = stats.double().reshape(2, n, case.rows // n, cout).sum(2)
    yd = y.double()
    s1, s2 = yd.sum((1, 2, 3)), (yd * yd).sum((1, 2, 3))
    es1 = ((per[0] - s1).abs() / yd.abs().sum((1, 2, 3)).clamp_min(1e-30)).max().item()
    es2 = ((per[1] - s2).abs() / s2.clamp_min(1e-30)).max().item()
    print("gauss", case.id, "sum y", es1, "sum y^2", es2)

    # the exact-fp32 path of the same convolution: it differs by the operand rounding, far above accumulation noise
    d32 = ops.conv3d_desc(tuple(xg.shape), cout, case.kd, (1, 1, 1), x_stride=r.xs)
    dense = ops.conv3d_desc(tuple(xg.shape), cout, case.kd, (1, 1, 1))
    wp32_f, wp32_d = ops.conv3d_pack(r.w)
    y32, _, _ = ops.conv3d_fwd(xg, wp32_f, d32, want_stats=False)
    dx32 = ops.conv3d_dgrad(dyg, wp32_d, dense)
    dw32 = ops.conv3d_wgrad(xg, dyg, d32)
    torch.cuda.synchronize()
    diffs = [_err(got, exact.double(), mag) for got, exact, mag in ((y, y32, y_mag), (dx, dx32, dx_mag), (dw, dw32, dw_mag))]
    print("gauss", case.id, "bf16 - fp32: y", diffs[0], "dx", diffs[1], "dw", diffs[2])

    assert ey < 2e-5 and edx < 2e-5 and edw < 2e-5, (ey, edx, edw)
    assert es1 < 1e-5 and es2 < 1e-5, (es1, es2)
    for diff, e in zip(diffs, (ey, edx, edw)):
        assert diff > 3e-5 and diff > 5 * e, (diff, e)
    r.dw_again_and_on_a_side_stream(ops, dw, case.id + " gauss")


REFUSALS = [
    # what, (N, D, H, W, Cin, Cout, kd, sd, shw), misaligned workspace, expected return code
    ("stride (1,2,2)", (1, 2, 8, 16, 64, 64, 3, 1, 2), False, E_UNSUPPORTED),
    ("Cin = 48", (1, 2, 8, 16, 48, 64, 3, 1, 1), False, E_UNSUPPORTED),
    ("kd = 3 with depth stride 2", (1, 2, 8, 16, 64, 64, 3, 2, 1), False, E_UNSUPPORTED),
    ("misaligned workspace", (1, 2, 8, 16, 64, 64, 3, 1, 1), True, E_BADARG),
]


@pytest.mark.parametrize("entry", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("what,shape,misaligned,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(ops, what, shape, misaligned, code, entry):
    """Every refusal is a host-side return before any launch: the expected code, an empty trace, outputs untouched."""
    L = lib()
    n, dd, h, w, cin, cout, kd, sd, shw = shape
    d = ops.conv3d_desc((n, dd, h, w, cin), cout, kd, (sd, shw, shw))
    ok = ops.conv3d_desc((n, dd, h, w, 64), 64, 3, (1, 1, 1))
    nws = L.unetk_conv3d_ws_bytes_bf16(ctypes.byref(ok))
    assert nws > 0 and (misaligned or L.unetk_conv3d_ws_bytes_bf16(ctypes.byref(d)) == 0)
    assert misaligned or L.unetk_conv3d_stat_rows_bf16(ctypes.byref(d)) == E_UNSUPPORTED
    sent = 12345.0
    vox = n * dd * h * w
    xbuf = torch.zeros(vox * cin, device="cuda")
    ybuf = torch.zeros(vox * cout, device="cuda")
    wbuf = torch.zeros(kd * 9 * cin * cout, device="cuda")
    out = torch.full((max(xbuf.numel(), ybuf.numel(), wbuf.numel()) + 64,), sent, device="cuda")
    out2 = torch.full((2 * 64 * cout,), sent, device="cuda")
    ws = torch.zeros(nws + 64, dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() + (4 if misaligned else 0)
    if entry == "fwd":
        call = lambda: L.unetk_conv3d_fwd_bf16(ctypes.byref(d), _p(xbuf), _p(wbuf), _p(out), _p(out2), _p(wsp), nws, _stream())
    elif entry == "dgrad":
        call = lambda: L.unetk_conv3d_dgrad_bf16(ctypes.byref(d), _p(ybuf), _p(wbuf), _p(out), _p(wsp), nws, _stream())
    else:
        call = lambda: L.unetk_conv3d_wgrad_bf16(ctypes.byref(d), _p(xbuf), _p(ybuf), _p(out), _p(wsp), nws, _stream())
    rc, names = _trace(ops, call)
    assert rc == code, (what, entry, rc, code)
    assert names == [], names
    assert bool((out == sent).all()) and bool((out2 == sent).all())


def _names_of(ops, case):
    if case.id not in TRACED:
        run_exact(ops, case, "eighths")
    return TRACED[case.id]


def test_table_reaches_every_required_kernel(ops):
    """From the traces themselves: all five tile shapes with the depth taps fused, each as a forward with statistics and as an
    input gradient (dstep = -1), and without; all four bf16 filter-gradient panels with kd = 3 and kd = 1; kd = 3 with one
    split and no slab_reduce launch, and with slab_reduce."""
    traces = [(c, _names_of(ops, c)) for c in CASES]
    for cfg in range(5):
        assert any(t["fwd"] == [T.bf(cfg, True)] for c, t in traces if c.kd == 3), ("forward", cfg)
        assert any(t["dgrad"] == [T.bf(cfg, True)] for c, t in traces if c.kd == 3), ("input gradient", cfg)
        assert any(T.bf(cfg, False) in t["fwd"] + t["dgrad"] for c, t in traces if c.kd == 1), ("kd = 1", cfg)
    for cit in (64, 32):
        for cot in (64, 32):
            for kd in (3, 1):
                assert any(t["wgrad"][0] == T.wg(cit, cot) for c, t in traces if c.kd == kd), (cit, cot, kd)
    assert any(len(t["wgrad"]) == 1 for c, t in traces if c.kd == 3)
    assert any(len(t["wgrad"]) == 2 and t["wgrad"][1].startswith("slab_reduce_kernel<") for c, t in traces if c.kd == 3)
