"""The edges of every buffer a kernel touches: outputs, statistic rows and workspaces (include/unetk.h contracts).

The parity tests reach the kernels through the ops.py wrappers, whose outputs are exact-size torch.empty tensors and whose
workspace is one reused, over-sized buffer -- so a write past the end of a view, into the channels beside a concat slice, a
statistic row never written, a workspace used beyond its *_ws_bytes() size or read before it is written all pass them unseen.
Here every call goes straight to the C ABI with guarded buffers (tests/guardbuf.py) and, per call:

  1. the outputs against a float64 reference on the device (bf16 modes: float64 on the bf16-rounded operands), at the
     tolerances of the op's parity test;
  2. every element outside every output view is bit-unchanged (guards, neighbour channels, the skip half of a concat);
  3. outputs the header declares fully written (y, dx, dw, stat rows [0, stat_rows) of both halves) hold no sentinel;
  4. read-only inputs, packed filters included, are bit-unchanged;
  5. the workspace filled with zeros, 0xFF (NaN) and 0x5F5F5F5F gives bitwise-equal outputs (this is also the determinism
     check of the split-K filter gradients and the statistic partials), and its guard stays intact;
  6. ws = NULL and a workspace 16 bytes short: the documented error code, or 1-4 pass;
and each case-table row asserts, through the library's launch trace, the kernel template it exists to reach.
"""
import ctypes
import math

import pytest
import torch

from guardbuf import GuardedWorkspace, guarded, guarded_input
from oracle import tf_ops

pytestmark = pytest.mark.gpu

E_BADARG, E_WORKSPACE = -1, -3
FILLS = (0x00, 0xFF, 0x5F)


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(x):
    """Device pointer of a guarded buffer / tensor / raw int (None -> NULL)."""
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    return ctypes.c_void_p(x.ptr() if hasattr(x, "ptr") else x.data_ptr())


def rel(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _r(t):
    """The bf16 values an fp32 tensor rounds to (RNE), as float64."""
    return t.float().bfloat16().double()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the per-call checker
def _trace(fn):
    from boxsegliver_amd import ops
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        rc = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return rc, ops.profile_read()[1]


def _edges(tag, outs, full, ins, inout):
    for name, o in outs.items():
        assert o.changed_outside() == 0, "{}: {} elements outside output `{}` changed".format(tag, o.changed_outside(), name)
    for name in full:
        assert outs[name].unwritten() == 0, "{}: {} elements of `{}` never written".format(tag, outs[name].unwritten(), name)
    for name, i in ins.items():
        assert i.changed_anywhere() == 0, "{}: read-only input `{}` changed".format(tag, name)
    for name, i in inout.items():
        assert i.changed_outside() == 0, "{}: elements outside in/out `{}` changed".format(tag, name)


def run_checked(launch, outs, ins, ws_bytes, verify, full=None, kernels=(), absent=(), inout=None, null_rc=(E_BADARG,),
                short_rc=(E_WORKSPACE,)):
    """launch(ws_ptr, ws_bytes) -> return code; outs / ins / inout: name -> Guarded; verify(dict of output clones) asserts
    the values.  null_rc / short_rc: the documented error codes of a NULL / a 16-byte short workspace (None: not offered).
    kernels: substrings each of which names a launched kernel; absent: substrings no launched kernel may contain."""
    full = list(outs) if full is None else list(full)
    inout = inout or {}
    ws = GuardedWorkspace(ws_bytes)

    def fresh():
        for o in list(outs.values()) + list(inout.values()):
            o.reset()

    def grab():
        return {n: o.view.clone() for n, o in outs.items()}

    first = names = None
    for k, byte in enumerate(FILLS if ws_bytes else FILLS[:2]):
        fresh()
        ws.fill(byte)
        tag = "ws fill 0x{:02X}".format(byte)
        if k == 0:
            rc, names = _trace(lambda: launch(P(ws.ptr()), ws.nbytes))
        else:
            rc = launch(P(ws.ptr()), ws.nbytes)
            torch.cuda.synchronize()
        assert rc == 0, "{}: return code {}".format(tag, rc)
        _edges(tag, outs, full, ins, inout)
        assert ws.guard_intact(), "{}: the workspace was used beyond its {} bytes".format(tag, ws_bytes)
        got = grab()
        if first is None:
            first = got
            verify(got)
        else:
            for n in got:
                assert torch.equal(_bits(got[n]), _bits(first[n])), "{}: `{}` differs from the first run".format(tag, n)
    for kern in kernels:
        assert any(kern in nm for nm in names), "no launch of {} among {}".format(kern, names)
    for kern in absent:
        assert not any(kern in nm for nm in names), "unexpected launch of {} among {}".format(kern, names)
    if ws_bytes and null_rc is not None:
        fresh()
        rc = launch(None, 0)
        torch.cuda.synchronize()
        if rc == 0:
            _edges("ws NULL", outs, full, ins, inout)
            verify(grab())
        assert rc == 0 or rc in null_rc, "ws NULL: return code {}".format(rc)
    if ws_bytes > 16 and short_rc is not None:
        short = GuardedWorkspace(ws_bytes - 16)
        short.fill(0x5F)
        fresh()
        rc = launch(P(short.ptr()), short.nbytes)
        torch.cuda.synchronize()
        assert short.guard_intact(), "short ws: used beyond its {} bytes".format(short.nbytes)
        if rc == 0:
            _edges("short ws", outs, full, ins, inout)
            verify(grab())
        assert rc == 0 or rc in short_rc, "short ws: return code {}".format(rc)
    return first, names


def stats_ok(s, ref, n_groups=1, atol_k=2e-4, rtol=2e-5):
    """Column sums of the statistic partials [2][rows][C] (each group's rows contiguous) against y's per-group moments."""
    s = s.double()
    rows, c = s.shape[1], s.shape[2]
    assert rows % n_groups == 0
    per = s.reshape(2, n_groups, rows // n_groups, c).sum(2)
    r = ref.double().reshape(n_groups, -1, c)
    s1, s2 = r.sum(1), (r * r).sum(1)
    assert (per[0] - s1).abs().max().item() <= atol_k * max(1.0, r.abs().sum(1).max().item())
    assert ((per[1] - s2).abs() / s2.abs().clamp_min(1e-30)).max().item() <= rtol


# ------------------------------------------------------------------------------------------------ conv3x3, fp32
IGEMM = "conv3x3_igemm_kernel<"
LIN = "conv3x3_igemm_lin_kernel<"
LIN_PLAIN = LIN + "4, 1, 1, 2, false, false, false, false, false, false>"        # 128-pixel blocks x 64 couts
LIN_SK = LIN + "2, 2, 2, 2, false, false, true, false, false, false>"          # stream-K, 128 x 128
SK = "lin_sk_fixup_kernel<128, 128>"
WG = "conv3x3_wgrad_kernel<"
WG64 = WG + "64, 64, false, 8, 16, false, 1, 1>"
WG32x64 = WG + "32, 64, false, 8, 16, false, 1, 1>"
BF = "conv3x3_igemm_bf16_kernel<"

# name, (N, H, W, Cin, Cout), x pixel-stride extra, y pixel-stride extra, dilation, fwd kernel, dgrad kernel (None: no dgrad),
# filter-gradient kernel.  The dgrad contracts Cout into Cin: it takes the forward's dispatch with the two swapped.
CONV_ROWS = [
    ("cfg0_8row", (4, 56, 224, 128, 128), 16, 64, 1, IGEMM + "2, 2, 2, 2, 1, 1, 0>", IGEMM + "2, 2, 2, 2, 1, 1, 0>", WG64),
    ("cfg0_small_grid", (1, 16, 48, 128, 128), 0, 0, 1, IGEMM + "2, 2, 1, 2, 1, 1, 0>", IGEMM + "2, 2, 1, 2, 1, 1, 0>", WG64),
    ("cfg0_big_grid", (2, 256, 256, 128, 128), 0, 0, 1, IGEMM + "2, 2, 4, 2, 1, 1, 0>", IGEMM + "2, 2, 4, 2, 1, 1, 0>", WG64),
    ("cfg1", (2, 16, 48, 32, 64), 32, 64, 1, IGEMM + "4, 1, 1, 2, 1, 1, 0>", IGEMM + "4, 1, 2, 1, 1, 1, 0>", WG32x64),
    ("cfg2", (2, 16, 48, 32, 32), 0, 32, 1, IGEMM + "4, 1, 2, 1, 1, 1, 0>", IGEMM + "4, 1, 2, 1, 1, 1, 0>",
     WG + "32, 32, false, 8, 16, false, 1, 1>"),
    ("lin", (2, 24, 24, 32, 64), 32, 64, 1, LIN_PLAIN, IGEMM + "4, 1, 2, 1, 1, 1, 0>", WG32x64),
    ("lin_streamk", (8, 16, 16, 128, 128), 0, 128, 1, LIN_SK, LIN_SK, WG64),
    ("c3_first_layer", (2, 24, 40, 3, 64), 0, 64, 1, "conv3x3_c3_mfma_kernel<3, float, false>", None,
     "conv3x3_wgrad_c3_kernel<64>"),
    ("direct_first_layer", (2, 20, 36, 3, 32), 0, 32, 1, "conv3x3_direct_kernel<3, float>", None, "conv3x3_wgrad_c3_kernel<32>"),
    ("dilation2", (2, 16, 40, 64, 64), 0, 64, 2, IGEMM + "4, 1, 1, 2, 1, 2, 0>", IGEMM + "4, 1, 1, 2, 1, 2, 0>",
     WG + "64, 64, false, 6, 16, false, 1, 2>"),
]


def _conv_desc(n, h, w, cin, cout, xs, ys, prec=0, dil=1):
    from boxsegliver_amd._abi import ConvDesc
    return ConvDesc(n, h, w, cin, cout, xs, ys, prec, dil if dil > 1 else 0)


def _coff(extra, align):
    return min(extra, align) if extra else 0


def _conv2d_ref(x, w, dy, dil=1):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = tf_ops.conv_nd_same(x64, w64, dilation=dil)
    dx, dw = torch.autograd.grad(y, (x64, w64), dy.double())
    return y.detach(), dx, dw


@pytest.mark.parametrize("row", CONV_ROWS, ids=[r[0] for r in CONV_ROWS])
def test_conv3x3_fp32_edges(ops, row):
    name, (n, h, w, cin, cout), xe, ye, dil, k_fwd, k_dgrad, k_wgrad = row
    g = _gen(n * 7 + h + cin + cout)
    x = torch.randn((n, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * cin)
    dy = torch.randn((n, h, w, cout), generator=g, device="cuda")
    y_ref, dx_ref, dw_ref = _conv2d_ref(x, wt, dy, dil)
    xs, ys = cin + xe, cout + ye
    xc, yc = _coff(xe, 8), _coff(ye, 16)
    d = _conv_desc(n, h, w, cin, cout, xs, ys, 0, dil)
    mfma = cin % 16 == 0 and cout % 32 == 0
    if mfma:
        wp_f, wp_d = ops.conv3x3_pack(wt)
    else:
        wp_f, wp_d = wt.contiguous(), None
    tol_y, tol_g = (1e-5, 1e-5) if dil > 1 else (2e-6, 3e-6)

    # forward + statistic partials
    gx, gw = guarded_input(x, xs, xc), guarded_input(wp_f.reshape(-1, 4) if mfma else wt)
    rows = lib().unetk_conv3x3_stat_rows(ctypes.byref(d))
    assert rows > 0
    gy, gs = guarded((n, h, w, cout), pixel_stride=ys, coff=yc), guarded((2, rows, cout))
    ws = lib().unetk_conv3x3_ws_bytes(ctypes.byref(d))
    if name == "lin_streamk":
        assert ws > 0
    if name == "lin":
        assert ws == 0

    def fwd(wsp, nb):
        return lib().unetk_conv3x3_fwd_ws(ctypes.byref(d), P(gx), P(gw), P(gy), P(gs), wsp, nb, stream())

    def v_fwd(o):
        assert rel(o["y"], y_ref) < tol_y
        if dil > 1:
            assert rel(o["stats"][0].double().sum(0), y_ref.sum((0, 1, 2))) < 1e-5
            assert rel(o["stats"][1].double().sum(0), (y_ref ** 2).sum((0, 1, 2))) < 1e-5
        else:
            stats_ok(o["stats"], y_ref)

    # the stream-K schedule is what the workspace buys: its fix-up kernel runs exactly when the shape has a workspace
    sk = (SK,) if name == "lin_streamk" else ()
    run_checked(fwd, {"y": gy, "stats": gs}, {"x": gx, "w": gw}, ws, v_fwd, kernels=(k_fwd,) + sk,
                absent=(SK,) if name == "lin" else (), null_rc=(), short_rc=())

    # input gradient (dy pixel stride y_stride, dx pixel stride x_stride)
    if k_dgrad is not None:
        gdy, gwd = guarded_input(dy, ys, yc), guarded_input(wp_d.reshape(-1, 4))
        gdx = guarded((n, h, w, cin), pixel_stride=xs, coff=xc)

        def dgrad(wsp, nb):
            return lib().unetk_conv3x3_dgrad_ws(ctypes.byref(d), P(gdy), P(gwd), P(gdx), wsp, nb, stream())

        run_checked(dgrad, {"dx": gdx}, {"dy": gdy, "w": gwd}, ws, lambda o: _lt(rel(o["dx"], dx_ref), tol_g),
                    kernels=(k_dgrad,) + sk, null_rc=(), short_rc=())

    # filter gradient: split-K through fixed-order slabs
    gx2, gdy2 = guarded_input(x, xs, xc), guarded_input(dy, ys, yc)
    gdw = guarded((3, 3, cin, cout))
    wws = lib().unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(d))

    def wgrad(wsp, nb):
        return lib().unetk_conv3x3_wgrad(ctypes.byref(d), P(gx2), P(gdy2), P(gdw), wsp, nb, stream())

    run_checked(wgrad, {"dw": gdw}, {"x": gx2, "dy": gdy2}, wws, lambda o: _lt(rel(o["dw"], dw_ref), tol_g),
                kernels=(k_wgrad,))


def _lt(a, b):
    assert a < b, (a, b)


# ------------------------------------------------------------------------------------------------ inference epilogue
AFFINE_ROWS = [
    ("tiled_pool", (2, 16, 48, 32, 128), True, IGEMM + "2, 2, 1, 2, 1, 1, 4>"),
    ("tiled", (2, 16, 48, 32, 128), False, IGEMM + "2, 2, 1, 2, 1, 1, 3>"),
    ("lin", (8, 16, 16, 128, 128), False, LIN_SK),
    ("c3_first_layer", (2, 24, 40, 3, 64), False, "conv3x3_c3_mfma_kernel<3, float, true>"),
]


@pytest.mark.parametrize("row", AFFINE_ROWS, ids=[r[0] for r in AFFINE_ROWS])
def test_conv3x3_fwd_affine_edges(ops, row):
    name, (n, h, w, cin, cout), pool, kern = row
    g = _gen(h * w + cin)
    x = torch.randn((n, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * cin)
    scale = torch.rand(cout, generator=g, device="cuda") + 0.5
    shift = torch.randn(cout, generator=g, device="cuda") * 0.1
    y_ref, _, _ = _conv2d_ref(x, wt, torch.zeros((n, h, w, cout), device="cuda"))
    z_ref = torch.relu(y_ref * scale.double() + shift.double())
    ys = cout + 64
    d = _conv_desc(n, h, w, cin, cout, cin, ys)
    assert lib().unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 1 if pool else 0) == 1
    mfma = cin % 16 == 0
    wsrc = ops.conv3x3_pack(wt)[0] if mfma else wt
    gx, gw = guarded_input(x), guarded_input(wsrc.reshape(-1, 4))
    gsc, gsh = guarded_input(scale), guarded_input(shift)
    gz = guarded((n, h, w, cout), pixel_stride=ys, coff=32)
    outs = {"z": gz}
    ps = cout + 32
    if pool:
        outs["pooled"] = gp = guarded((n, h // 2, w // 2, cout), pixel_stride=ps, coff=0)
    ws = lib().unetk_conv3x3_ws_bytes(ctypes.byref(d))

    def launch(wsp, nb):
        return lib().unetk_conv3x3_fwd_affine(ctypes.byref(d), P(gx), P(gw), P(gsc), P(gsh), P(gz),
                                              P(gp) if pool else None, ps if pool else 0, wsp, nb, stream())

    def verify(o):
        assert rel(o["z"], z_ref) < 2e-6
        if pool:
            zz = o["z"].reshape(n, h // 2, 2, w // 2, 2, cout)
            assert torch.equal(o["pooled"], zz.amax((2, 4)))

    run_checked(launch, outs, {"x": gx, "w": gw, "scale": gsc, "shift": gsh}, ws, verify, kernels=(kern,), null_rc=(),
                short_rc=())


def test_conv3x3_dgrad_nbr_edges(ops):
    """conv2's input gradient fused with conv1's norm-backward reduction: dx and the partials [2][rows][Cin]."""
    n, h, w, cin, cout = 2, 16, 48, 128, 128
    g = _gen(11)
    wt = torch.randn((3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * cin)
    dy = torch.randn((n, h, w, cout), generator=g, device="cuda")
    prod_y = torch.randn((n, h, w, cin), generator=g, device="cuda")
    mean = prod_y.double().mean((0, 1, 2))
    rstd = 1.0 / torch.sqrt(prod_y.double().var((0, 1, 2), unbiased=False) + 1e-3)
    gamma = torch.rand(cin, generator=g, device="cuda").double() + 0.5
    beta = torch.randn(cin, generator=g, device="cuda").double() * 0.1
    scale, shift = gamma * rstd, beta - mean * gamma * rstd
    _, dx_ref, _ = _conv2d_ref(torch.zeros((n, h, w, cin), device="cuda"), wt, dy)
    pys = cin + 64
    d = _conv_desc(n, h, w, cin, cout, cin, cout)
    rows = lib().unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(d))
    assert rows > 0
    _, wp_d = ops.conv3x3_pack(wt)
    gdy, gw = guarded_input(dy), guarded_input(wp_d.reshape(-1, 4))
    gpy = guarded_input(prod_y, pys, 32)
    gin = {n_: guarded_input(t.float()) for n_, t in (("scale", scale), ("shift", shift), ("mean", mean), ("rstd", rstd))}
    gdx, gpart = guarded((n, h, w, cin)), guarded((2, rows, cin))

    def launch(wsp, nb):
        return lib().unetk_conv3x3_dgrad_nbr(ctypes.byref(d), P(gdy), P(gw), P(gdx), P(gpy), pys, P(gin["scale"]),
                                             P(gin["shift"]), P(gin["mean"]), P(gin["rstd"]), 0, P(gpart), stream())

    def verify(o):
        assert rel(o["dx"], dx_ref) < 3e-6
        # partials of the device's own dx: sum du and sum du * xhat, du = dx * (prod_y * scale + shift > 0)
        dx = o["dx"].double()
        py = prod_y.double()
        du = dx * ((py * scale.float().double() + shift.float().double()) > 0)
        xhat = (py - mean.float().double()) * rstd.float().double()
        p = o["partials"].double().sum(1)
        assert rel(p[0], du.sum((0, 1, 2))) < 1e-5
        assert rel(p[1], (du * xhat).sum((0, 1, 2))) < 1e-5

    ins = dict(gin, dy=gdy, w=gw, prod_y=gpy)
    run_checked(launch, {"dx": gdx, "partials": gpart}, ins, 0, verify, kernels=(IGEMM + "2, 2, 1, 2, 1, 1, 2>",))


# ------------------------------------------------------------------------------------------------ conv3x3, bf16 modes
def _stored_ok(got_bf16, ref64, flips=2e-3):
    """As test_gpu_bf16s: every element within one bf16 ulp of the exact result, all but `flips` rounded exactly."""
    got = got_bf16.double()
    err = (got - ref64).abs() / ref64.abs().clamp_min(1e-30)
    big = ref64.abs() > 1e-3 * ref64.abs().max()
    assert err[big].max().item() <= 1.01 * 2.0 ** -8, err[big].max().item()
    assert (got == _r(ref64.float())).double().mean().item() > 1.0 - flips


# name, precision, (N, H, W, Cin, Cout), fwd kernel, dgrad kernel, filter-gradient kernel.  UNETK_BF16 picks its tile by
# pick_bf16 (conv_igemm_bf16.hip): cfg 0 = 512 x 128 (H >= 24 and >= 200 blocks), 1 = 128 x 128, 2 = 256 x 64 (H >= 12),
# 3 = 128 x 64, 4 = 256 x 32.  UNETK_BF16S runs the persistent kernel (conv_igemm_bf16s.hip) where its 32 x 16 tiles number
# >= 200, else the BS instances of the same tiles (cfg 0 is then never chosen: it needs the same 200 tiles; cfg 4 is refused).
WGB = WG + "64, 64, true, 8, 16, false, 1, 1>"
BS_K = "conv3x3_bf16s_kernel<8, false, 0>"
WG_BS = "conv3x3_wgrad_bf16s_kernel<true>"
BF16_ROWS = [
    ("bf16_cfg0", 1, (4, 64, 400, 128, 128), BF + "4, 2, 4, 2, false, false, false>", BF + "4, 2, 4, 2, false, false, false>", WGB),
    ("bf16_cfg1", 1, (2, 16, 48, 64, 128), BF + "2, 2, 2, 2, false, false, false>", BF + "4, 1, 2, 2, false, false, false>", WGB),
    ("bf16_cfg2", 1, (2, 16, 48, 64, 64), BF + "4, 1, 2, 2, false, false, false>", BF + "4, 1, 2, 2, false, false, false>", WGB),
    ("bf16_cfg3", 1, (2, 8, 48, 64, 64), BF + "4, 1, 1, 2, false, false, false>", BF + "4, 1, 1, 2, false, false, false>", WGB),
    ("bf16_cfg4", 1, (2, 16, 48, 64, 32), BF + "4, 1, 2, 1, false, false, false>", BF + "4, 1, 2, 2, false, false, false>",
     WG + "64, 32, true, 8, 16, false, 1, 1>"),
    ("bf16s_persistent", 2, (4, 64, 400, 128, 128), BS_K, BS_K, WG_BS),
    ("bf16s_cfg1", 2, (2, 16, 48, 64, 128), BF + "2, 2, 2, 2, true, false, false>", BF + "4, 1, 2, 2, true, false, false>", WG_BS),
    ("bf16s_cfg2", 2, (2, 16, 48, 64, 64), BF + "4, 1, 2, 2, true, false, false>", BF + "4, 1, 2, 2, true, false, false>", WG_BS),
    ("bf16s_cfg3", 2, (2, 8, 48, 64, 64), BF + "4, 1, 1, 2, true, false, false>", BF + "4, 1, 1, 2, true, false, false>", WG_BS),
]


@pytest.mark.parametrize("row", BF16_ROWS, ids=[r[0] for r in BF16_ROWS])
def test_conv3x3_bf16_edges(ops, row):
    name, prec, (n, h, w, cin, cout), k_fwd, k_dgrad, k_wgrad = row
    g = _gen(prec * 101 + h + w + cin + cout)
    sdt = torch.bfloat16 if prec == 2 else torch.float32
    x = torch.randn((n, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * cin)
    dy = torch.randn((n, h, w, cout), generator=g, device="cuda")
    y_ref, dx_ref, dw_ref = _conv2d_ref(_r(x), _r(wt), _r(dy))
    xs, ys = cin + 64, cout + 64
    d = _conv_desc(n, h, w, cin, cout, xs, ys, prec)
    wp_f, wp_d = ops.conv3x3_pack(wt, bf16=prec)
    gx, gw = guarded_input(x, xs, 32, dtype=sdt), guarded_input(wp_f.reshape(-1, 8))
    rows = lib().unetk_conv3x3_stat_rows(ctypes.byref(d))
    gy, gs = guarded((n, h, w, cout), sdt, ys, 32), guarded((2, rows, cout))
    ws = lib().unetk_conv3x3_ws_bytes(ctypes.byref(d))
    assert ws == 0

    def v_fwd(o):
        if prec == 2:
            _stored_ok(o["y"], y_ref)
            stats_ok(o["stats"], y_ref, atol_k=3e-5, rtol=3e-5)
        else:
            assert rel(o["y"], y_ref) < 3e-6
            stats_ok(o["stats"], y_ref, atol_k=3e-4, rtol=3e-5)

    run_checked(lambda wsp, nb: lib().unetk_conv3x3_fwd_ws(ctypes.byref(d), P(gx), P(gw), P(gy), P(gs), wsp, nb, stream()),
                {"y": gy, "stats": gs}, {"x": gx, "w": gw}, ws, v_fwd, kernels=(k_fwd,))
    gdy, gwd = guarded_input(dy, ys, 32, dtype=sdt), guarded_input(wp_d.reshape(-1, 8))
    gdx = guarded((n, h, w, cin), sdt, xs, 32)

    def v_dgrad(o):
        if prec == 2:
            _stored_ok(o["dx"], dx_ref)
        else:
            assert rel(o["dx"], dx_ref) < 3e-6

    run_checked(lambda wsp, nb: lib().unetk_conv3x3_dgrad_ws(ctypes.byref(d), P(gdy), P(gwd), P(gdx), wsp, nb, stream()),
                {"dx": gdx}, {"dy": gdy, "w": gwd}, ws, v_dgrad, kernels=(k_dgrad,))
    gdw = guarded((3, 3, cin, cout))
    wws = lib().unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(d))
    run_checked(lambda wsp, nb: lib().unetk_conv3x3_wgrad(ctypes.byref(d), P(gx), P(gdy), P(gdw), wsp, nb, stream()),
                {"dw": gdw}, {"x": gx, "dy": gdy}, wws, lambda o: _lt(rel(o["dw"], dw_ref), 1e-5 if prec == 2 else 5e-6),
                kernels=(k_wgrad,))


def test_conv3x3_bf16s_first_layer_edges(ops):
    """UNETK_BF16S first layer: fp32 image in (x_stride = Cin = 3), bf16 out into a concat slice."""
    n, h, w, cin, cout = 2, 40, 52, 3, 64
    g = _gen(3)
    x = torch.rand((n, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(27)
    dy = torch.randn((n, h, w, cout), generator=g, device="cuda").bfloat16()
    y_ref, _, dw_ref = _conv2d_ref(x, wt, dy.double())
    ys = cout + 64
    d = _conv_desc(n, h, w, cin, cout, cin, ys, 2)
    gx, gw = guarded_input(x), guarded_input(wt)
    rows = lib().unetk_conv3x3_stat_rows(ctypes.byref(d))
    gy, gs = guarded((n, h, w, cout), torch.bfloat16, ys, 64), guarded((2, rows, cout))

    def v_fwd(o):
        _stored_ok(o["y"], y_ref)
        ref = y_ref
        assert (o["stats"].double()[0].sum(0) - ref.sum((0, 1, 2))).abs().max().item() < \
            1e-4 * ref.abs().sum((0, 1, 2)).max().item()

    run_checked(lambda wsp, nb: lib().unetk_conv3x3_fwd_ws(ctypes.byref(d), P(gx), P(gw), P(gy), P(gs), wsp, nb, stream()),
                {"y": gy, "stats": gs}, {"x": gx, "w": gw}, 0, v_fwd, kernels=("conv3x3_c3_mfma_kernel<3, unsigned short, false>",))
    gdy, gdw = guarded_input(dy, ys, 64), guarded((3, 3, cin, cout))
    wws = lib().unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(d))
    run_checked(lambda wsp, nb: lib().unetk_conv3x3_wgrad(ctypes.byref(d), P(gx), P(gdy), P(gdw), wsp, nb, stream()),
                {"dw": gdw}, {"x": gx, "dy": gdy}, wws, lambda o: _lt(rel(o["dw"], dw_ref), 1e-5),
                kernels=("conv3x3_wgrad_c3_bf16s_kernel(",))


# ------------------------------------------------------------------------------------------------ conv3d
def _conv3d_desc(n, dd, h, w, cin, cout, kd, sd, shw, xs, ys, cin_live8=0):
    from boxsegliver_amd._abi import Conv3dDesc
    d = Conv3dDesc(n, dd, h, w, cin, cout, kd, sd, shw, xs, ys)
    d.cin_live8[0], d.cin_live8[1] = cin_live8 & 0xFFFFFFFF, (cin_live8 >> 32) & 0xFFFFFFFF
    return d


def _out_dims(d):
    do, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib().unetk_conv3d_out_dims(ctypes.byref(d), ctypes.byref(do), ctypes.byref(ho), ctypes.byref(wo)) == 0
    return do.value, ho.value, wo.value


S2D, SUB = "s2d_kernel", "subsample2_stats_kernel"

# name, (N, D, H, W, Cin, Cout, kd, sd, shw), x extra, y extra, live channels of Cin (None: all), fwd kernels, dgrad kernels
# (None: not run), wgrad kernels (None: not run)
LIN_GEN4 = LIN + "4, 1, 1, 1, true, true, false, false, false, false>"     # stride-2 dgrad: four parity classes in one block
LIN_GRP = LIN + "4, 1, 1, 2, false, false, false, false, true, false>"     # grouped taps over the space-to-depth copy
WG_S2 = WG + "32, 64, false, 4, 16, false, 2, 1>"                          # natively strided filter gradient
CONV3D_ROWS = [
    ("kd1_tiled", (2, 3, 12, 40, 32, 64, 1, 1, 1), 32, 64, None, (IGEMM + "4, 1, 1, 2, 1, 1, 0>",),
     (IGEMM + "4, 1, 2, 1, 1, 1, 0>",), (WG32x64,)),
    ("kd3_tiled_taps", (1, 3, 8, 40, 32, 64, 3, 1, 1), 32, 64, None, ("zero_slice_kernel", IGEMM + "4, 1, 1, 2, 1, 1, 1>"),
     ("zero_slice_kernel", IGEMM + "4, 1, 2, 1, 1, 1, 1>"), (WG32x64,)),
    ("kd3_fused_lin", (2, 4, 12, 12, 32, 64, 3, 1, 1), 32, 64, None, (LIN_PLAIN,),
     ("zero_slice_kernel", IGEMM + "4, 1, 2, 1, 1, 1, 1>"), (WG32x64,)),
    ("kd3_live8", (2, 4, 12, 12, 64, 64, 3, 1, 1), 0, 0, 40, (LIN_PLAIN,), (LIN_PLAIN,), None),
    ("s2lin_sd1", (2, 4, 12, 12, 32, 64, 3, 1, 2), 32, 64, None, (S2D, LIN_GRP), (LIN_GEN4,),
     (WG + "32, 64, false, 4, 6, false, 2, 1>",)),
    ("s2lin_sd2", (2, 6, 12, 12, 64, 128, 3, 2, 2), 0, 0, None, (S2D, LIN + "2, 2, 2, 2, false, false, false, false, true, false>"),
     (LIN + "4, 1, 1, 2, true, true, false, false, false, false>",), (WG + "32, 64, false, 4, 6, false, 2, 1>",)),
    ("native_s2_th4", (1, 2, 8, 66, 32, 128, 1, 1, 2), 16, 0, None, (IGEMM + "2, 2, 1, 2, 2, 1, 0>",), (LIN_GEN4,), (WG_S2,)),
    ("native_s2_th8", (1, 2, 8, 66, 32, 64, 1, 1, 2), 0, 64, None, (IGEMM + "4, 1, 1, 2, 2, 1, 0>",), (LIN_GEN4,), (WG_S2,)),
    ("native_s2_kd3", (1, 4, 8, 66, 32, 64, 3, 2, 2), 0, 0, None, (IGEMM + "4, 1, 1, 2, 2, 1, 0>",), (LIN_GEN4,), (WG_S2,)),
    ("subsample_fallback", (1, 2, 8, 12, 32, 32, 1, 1, 2), 0, 32, None, (IGEMM + "4, 1, 2, 1, 1, 1, 0>", SUB), (LIN_GEN4,),
     ("dilate2_kernel", WG + "32, 32, false, 8, 16, false, 1, 1>")),
    ("first_layer", (2, 4, 16, 40, 1, 32, 3, 1, 1), 0, 32, None, ("zero_slice_kernel", "conv3x3_direct_kernel<1, float>"), None,
     ("conv3x3_wgrad_c3_kernel<32>",)),
    # the filter gradient runs one launch per depth tap, and taps 0 and 2 reach 7 of the 8 planes: 504 tiles in 504 splits of
    # one tile, where the 576 tiles of all 8 planes make 288 splits of two (the split count is not monotone in the tiles).
    # The workspace query has to size the slabs of the launches that run, not of a launch over every plane.
    ("first_layer_resplit", (1, 8, 96, 96, 1, 32, 3, 1, 1), 0, 0, None, ("conv3x3_direct_kernel<1, float>",), None,
     ("conv3x3_wgrad_c3_kernel<32>",)),
    # the input gradient's fallback for dy planes the four-class kernel refuses (conv3d.hip DGRAD_DILATED): dy zero-dilated
    # into the workspace, dx zeroed, one accumulating stride-1 launch per depth tap -- dy planes 8 x 80, 4 x 112 and 2 x 1
    ("dgrad_dilated_w80", (1, 2, 16, 160, 32, 64, 1, 1, 2), 32, 64, None, (IGEMM + "4, 1, 1, 2, 2, 1, 0>",),
     ("dilate2_kernel", IGEMM + "4, 1, 2, 1, 1, 1, 0>"), (WG_S2,)),
    ("dgrad_dilated_w112_kd3", (1, 3, 8, 224, 64, 64, 3, 1, 2), 0, 0, None, (IGEMM + "4, 1, 1, 2, 2, 1, 0>",),
     ("dilate2_kernel", IGEMM + "4, 1, 1, 2, 1, 1, 1>"), (WG_S2,)),
    ("dgrad_dilated_2x1_sd2", (1, 4, 4, 2, 64, 64, 3, 2, 2), 32, 0, None, (IGEMM + "4, 1, 1, 2, 2, 1, 0>",),
     ("dilate2_kernel", "zero_slice_kernel", LIN + "4, 1, 1, 2, false, false, false, true, false, false>",
      IGEMM + "4, 1, 1, 2, 1, 1, 1>"), (WG_S2,)),
]


@pytest.mark.parametrize("row", CONV3D_ROWS, ids=[r[0] for r in CONV3D_ROWS])
def test_conv3d_fp32_edges(ops, row):
    name, (n, dd, h, w, cin, cout, kd, sd, shw), xe, ye, live, kernels, k_dgrad, k_wgrad = row
    g = _gen(n + dd * 3 + h + cin * 5 + cout + kd + sd * 7 + shw)
    x = torch.randn((n, dd, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((kd, 3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * kd * cin)
    mask = 0
    if live is not None:        # a channel-padded layer: the filter rows of the padding are zero, the promise says so
        wt[:, :, :, live:, :] = 0
        mask = sum(1 << i for i in range((live + 7) // 8))
    xs, ys = cin + xe, cout + ye
    xc, yc = _coff(xe, 16), _coff(ye, 32)
    d = _conv3d_desc(n, dd, h, w, cin, cout, kd, sd, shw, xs, ys, mask)
    do, ho, wo = _out_dims(d)
    dy = torch.randn((n, do, ho, wo, cout), generator=g, device="cuda")
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = tf_ops.conv_nd_same(x64, w64, stride=(sd, shw, shw))
    dx_ref, dw_ref = torch.autograd.grad(y_ref, (x64, w64), dy.double())
    y_ref = y_ref.detach()
    mfma = cin % 4 == 0
    if mfma:
        wp_f, wp_d = ops.conv3d_pack(wt)
    else:
        wp_f, wp_d = wt.contiguous(), None
    ws = lib().unetk_conv3d_ws_bytes(ctypes.byref(d))
    rows = lib().unetk_conv3d_stat_rows(ctypes.byref(d))
    assert rows > 0
    gx, gw = guarded_input(x, xs, xc), guarded_input(wp_f.reshape(-1, 4) if mfma else wt)
    gy, gs = guarded((n, do, ho, wo, cout), pixel_stride=ys, coff=yc), guarded((2, rows, cout))
    # the forward refuses a missing or short workspace on every path that uses one (include/unetk.h): the space-to-depth copy
    # and the stride-1 conv + subsample
    needs_ws = S2D in kernels or SUB in kernels

    def fwd(wsp, nb):
        return lib().unetk_conv3d_fwd(ctypes.byref(d), P(gx), P(gw), P(gy), P(gs), wsp, nb, stream())

    def v_fwd(o):
        assert rel(o["y"], y_ref) < 3e-6
        stats_ok(o["stats"], y_ref, n_groups=n, atol_k=3e-4, rtol=3e-5)

    run_checked(fwd, {"y": gy, "stats": gs}, {"x": gx, "w": gw}, ws, v_fwd, kernels=kernels,
                null_rc=(E_BADARG,) if needs_ws else (), short_rc=(E_WORKSPACE,) if needs_ws else ())
    if needs_ws:     # and says so, rather than writing another number of statistic rows
        assert fwd(None, 0) == E_BADARG
        if ws > 16:
            short = GuardedWorkspace(ws - 16)
            assert fwd(P(short.ptr()), short.nbytes) == E_WORKSPACE
        torch.cuda.synchronize()

    if k_dgrad is not None:
        dense = _conv3d_desc(n, dd, h, w, cin, cout, kd, sd, shw, xs, ys, mask)
        gdy, gwd = guarded_input(dy, ys, yc), guarded_input(wp_d.reshape(-1, 4))
        gdx = guarded((n, dd, h, w, cin), pixel_stride=xs, coff=xc)
        run_checked(lambda wsp, nb: lib().unetk_conv3d_dgrad(ctypes.byref(dense), P(gdy), P(gwd), P(gdx), wsp, nb, stream()),
                    {"dx": gdx}, {"dy": gdy, "w": gwd}, ws, lambda o: _lt(rel(o["dx"], dx_ref), 5e-6), kernels=k_dgrad,
                    null_rc=(E_BADARG, E_WORKSPACE), short_rc=(E_WORKSPACE,))
    if k_wgrad is not None:
        gx2, gdy2 = guarded_input(x, xs, xc), guarded_input(dy, ys, yc)
        gdw = guarded((kd, 3, 3, cin, cout))
        run_checked(lambda wsp, nb: lib().unetk_conv3d_wgrad(ctypes.byref(d), P(gx2), P(gdy2), P(gdw), wsp, nb, stream()),
                    {"dw": gdw}, {"x": gx2, "dy": gdy2}, ws, lambda o: _lt(rel(o["dw"], dw_ref), 5e-6), kernels=k_wgrad,
                    null_rc=(E_BADARG, E_WORKSPACE), short_rc=(E_WORKSPACE,))


def _conv3d_bf16_ref(x, w, dy):
    """float64 on bf16-rounded operands and the magnitudes the accumulation noise scales with (test_gpu_unet3d_bf16c)."""
    xr, wr = _r(x).requires_grad_(True), _r(w).requires_grad_(True)
    y = tf_ops.conv_nd_same(xr, wr)
    dx, dw = torch.autograd.grad(y, (xr, wr), _r(dy))
    xa, wa = xr.detach().abs().requires_grad_(True), wr.detach().abs().requires_grad_(True)
    ya = tf_ops.conv_nd_same(xa, wa)
    dxa, dwa = torch.autograd.grad(ya, (xa, wa), _r(dy).abs())
    return y.detach(), dx, dw, ya.detach(), dxa, dwa


def _err(got, ref, mag):
    return ((got.double() - ref).abs() / mag.clamp_min(1e-30)).max().item()


# name, (N, D, H, W, Cin, Cout, kd), fwd kernel, dgrad kernel, wgrad kernel: the depth taps fused in one launch (template flag
# FT) for kd = 3, the plain 2-D instance for kd = 1
CONV3D_BF16_ROWS = [
    ("kd3_small", (2, 4, 12, 12, 32, 64, 3), BF + "4, 1, 2, 2, false, false, true>", BF + "4, 1, 2, 1, false, false, true>",
     WG + "32, 64, true, 8, 16, false, 1, 1>"),
    ("kd1", (1, 3, 8, 40, 64, 32, 1), BF + "4, 1, 2, 1, false, false, false>", BF + "4, 1, 1, 2, false, false, false>",
     WG + "64, 32, true, 8, 16, false, 1, 1>"),
]


@pytest.mark.parametrize("row", CONV3D_BF16_ROWS, ids=[r[0] for r in CONV3D_BF16_ROWS])
def test_conv3d_bf16_edges(ops, row):
    from boxsegliver_amd import _abi
    _, (n, dd, h, w, cin, cout, kd), k_fwd, k_dgrad, k_wgrad = row
    g = _gen(cin * 31 + cout + h + n)
    x = torch.randn((n, dd, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((kd, 3, 3, cin, cout), generator=g, device="cuda") / math.sqrt(9 * kd * cin)
    dy = torch.randn((n, dd, h, w, cout), generator=g, device="cuda")
    y_ref, dx_ref, dw_ref, y_mag, dx_mag, dw_mag = _conv3d_bf16_ref(x.double(), wt.double(), dy.double())
    xs, ys = cin + 32, cout + 32
    d = _conv3d_desc(n, dd, h, w, cin, cout, kd, 1, 1, xs, ys)
    dense = _conv3d_desc(n, dd, h, w, cin, cout, kd, 1, 1, xs, ys)
    wp_f, wp_d = ops.conv3d_pack(wt, precision=_abi.BF16)
    ws = lib().unetk_conv3d_ws_bytes_bf16(ctypes.byref(d))
    rows = lib().unetk_conv3d_stat_rows_bf16(ctypes.byref(d))
    assert ws > 0 and rows > 0
    gx, gw, gwd = guarded_input(x, xs, 16), guarded_input(wp_f.reshape(-1, 8)), guarded_input(wp_d.reshape(-1, 8))
    gdy = guarded_input(dy, ys, 16)
    gy, gs = guarded((n, dd, h, w, cout), pixel_stride=ys, coff=16), guarded((2, rows, cout))
    gdx, gdw = guarded((n, dd, h, w, cin), pixel_stride=xs, coff=16), guarded((kd, 3, 3, cin, cout))

    def v_fwd(o):
        assert _err(o["y"], y_ref, y_mag) < 2e-5
        per = o["stats"].double().reshape(2, n, rows // n, cout).sum(2)
        yd = o["y"].double()
        s1, s2 = yd.sum((1, 2, 3)), (yd * yd).sum((1, 2, 3))
        assert ((per[0] - s1).abs() / yd.abs().sum((1, 2, 3)).clamp_min(1e-30)).max().item() < 1e-5
        assert ((per[1] - s2).abs() / s2.clamp_min(1e-30)).max().item() < 1e-5

    run_checked(lambda wsp, nb: lib().unetk_conv3d_fwd_bf16(ctypes.byref(d), P(gx), P(gw), P(gy), P(gs), wsp, nb, stream()),
                {"y": gy, "stats": gs}, {"x": gx, "w": gw}, ws, v_fwd, kernels=(k_fwd,))
    run_checked(lambda wsp, nb: lib().unetk_conv3d_dgrad_bf16(ctypes.byref(dense), P(gdy), P(gwd), P(gdx), wsp, nb, stream()),
                {"dx": gdx}, {"dy": gdy, "w": gwd}, ws, lambda o: _lt(_err(o["dx"], dx_ref, dx_mag), 2e-5),
                kernels=(k_dgrad,))
    run_checked(lambda wsp, nb: lib().unetk_conv3d_wgrad_bf16(ctypes.byref(d), P(gx), P(gdy), P(gdw), wsp, nb, stream()),
                {"dw": gdw}, {"x": gx, "dy": gdy}, ws, lambda o: _lt(_err(o["dw"], dw_ref, dw_mag), 2e-5),
                kernels=(k_wgrad,))


# ------------------------------------------------------------------------------------------------ transposed convs
def _deconv_ref(x, w, b, kd):
    """out[n, kd z + e, 2y + a, 2x + c, co] = relu(sum_ci x[n, z, y, x, ci] w[e, a, c, co, ci] + b[co]); x [N, D, H, W, Cin]."""
    n, dd, h, ww, _ = x.shape
    cout = w.shape[3]
    t = torch.einsum("nzyxi,eacoi->nzeyaxco", x, w).reshape(n, dd * kd, 2 * h, 2 * ww, cout)
    return torch.relu(t + b) if b is not None else torch.relu(t)


# the transposed conv: one pointwise GEMM forward (mode 0), and backward = ReLU backward + bias gradient, the input-gradient GEMM
# (mode 1) and the filter gradient
DECONV_FWD = "pw_gemm_kernel<0, 2, 2, 2, 2>"
DECONV_BWD = ("relu_bwd_bias_kernel<float>", "pw_gemm_kernel<1, 4, 1, 1, 2>", "deconv_wgrad4_kernel(")


@pytest.mark.parametrize("kind", ["2d", "3d_kd2"])
def test_deconv_concat_edges(ops, kind):
    """Forward straight into the concat buffer at out_coff (the skip half present and untouched), backward, backward in
    two parts through the same workspace."""
    from boxsegliver_amd._abi import Deconv3dDesc, DeconvDesc
    if kind == "2d":
        n, dd, h, w, cin, cout, kd = 2, 1, 8, 12, 64, 32, 1
    else:
        n, dd, h, w, cin, cout, kd = 1, 3, 4, 6, 64, 32, 2
    skip = 32
    os_ = skip + cout
    g = _gen(cin + cout + kd)
    x = torch.randn((n, dd, h, w, cin), generator=g, device="cuda")
    wt = torch.randn((kd, 2, 2, cout, cin), generator=g, device="cuda") / math.sqrt(cin)
    b = torch.randn(cout, generator=g, device="cuda") * 0.1 if kind == "2d" else None
    oshape = (n, dd * kd, 2 * h, 2 * w, cout) if kind != "2d" else (n, 2 * h, 2 * w, cout)
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    up = _deconv_ref(x64, w64, b64, kd).reshape(oshape)
    dcat_full = torch.randn(oshape[:-1] + (os_,), generator=g, device="cuda")
    grads = torch.autograd.grad(up, [t for t in (x64, w64, b64) if t is not None], dcat_full[..., skip:].double())
    dx_ref, dw_ref = grads[0], grads[1]
    db_ref = grads[2] if b is not None else None
    xin = x.reshape((n, h, w, cin)) if kind == "2d" else x
    if kind == "2d":
        d = DeconvDesc(n, h, w, cin, cout, os_, skip, 0)
        wp_f, wp_d = ops.deconv2x2_pack(wt[0])
        fwd_fn, bwd_fn, parts_fn = lib().unetk_deconv2x2_fwd, lib().unetk_deconv2x2_bwd, lib().unetk_deconv2x2_bwd_parts
        ws = lib().unetk_deconv2x2_bwd_ws_bytes(ctypes.byref(d))
    else:
        d = Deconv3dDesc(n, dd, h, w, cin, cout, kd, os_, skip, 0)
        wp_f, wp_d = ops.deconv3d_pack(wt)
        fwd_fn, bwd_fn, parts_fn = lib().unetk_deconv3d_fwd, lib().unetk_deconv3d_bwd, lib().unetk_deconv3d_bwd_parts
        ws = lib().unetk_deconv3d_bwd_ws_bytes(ctypes.byref(d))
    skip_data = torch.randn(oshape[:-1] + (skip,), generator=g, device="cuda")

    def concat_out():
        o = guarded(oshape, pixel_stride=os_, coff=skip)
        o.flat.as_strided(oshape[:-1] + (skip,), o.strides[:-1] + (1,), o.guard).copy_(skip_data)
        o.snap = o.flat.clone()
        return o

    def base(o):
        return o.flat.data_ptr() + o.guard * 4

    gx, gwf, gwd = guarded_input(xin), guarded_input(wp_f.reshape(-1, 4)), guarded_input(wp_d.reshape(-1, 4))
    gb = guarded_input(b) if b is not None else None
    gcat = concat_out()
    ins = {"x": gx, "w": gwf}
    if gb is not None:
        ins["bias"] = gb
    fwd_res, _ = run_checked(lambda wsp, nb: fwd_fn(ctypes.byref(d), P(gx), P(gwf), P(gb), P(base(gcat)), stream()),
                             {"up": gcat}, ins, 0, lambda o: _lt(rel(o["up"], up.detach()), 3e-6), kernels=(DECONV_FWD,))

    # backward: the forward's concat buffer (value) and its gradient, both with the skip half beside the view
    cat_in = guarded_input(fwd_res["up"], os_, skip)
    dcat_in = guarded_input(dcat_full[..., skip:], os_, skip)
    gdx = guarded(xin.shape)
    gdw = guarded((kd, 2, 2, cout, cin)) if kind != "2d" else guarded((2, 2, cout, cin))
    outs = {"dx": gdx, "dw": gdw}
    if b is not None:
        outs["db"] = gdb = guarded((cout,))
    else:
        gdb = None
    bins = {"x": gx, "w": gwd, "cat": cat_in, "dcat": dcat_in}
    cat_base = cat_in.flat.data_ptr() + cat_in.guard * 4
    dcat_base = dcat_in.flat.data_ptr() + dcat_in.guard * 4

    def v_bwd(o):
        assert rel(o["dx"], dx_ref.reshape(o["dx"].shape)) < 5e-6
        assert rel(o["dw"], dw_ref.reshape(o["dw"].shape)) < 5e-6
        if db_ref is not None:
            assert rel(o["db"], db_ref) < 5e-6

    res, _ = run_checked(lambda wsp, nb: bwd_fn(ctypes.byref(d), P(gx), P(gwd), P(cat_base), P(dcat_base), P(gdx), P(gdw),
                                                P(gdb), wsp, nb, stream()), outs, bins, ws, v_bwd, kernels=DECONV_BWD)

    def two_parts(wsp, nb):
        rc = parts_fn(ctypes.byref(d), P(gx), P(gwd), P(cat_base), P(dcat_base), P(gdx), P(gdw), P(gdb), wsp, nb, 1, stream())
        if rc != 0:
            return rc
        return parts_fn(ctypes.byref(d), P(gx), P(gwd), P(cat_base), P(dcat_base), P(gdx), P(gdw), P(gdb), wsp, nb, 2,
                        stream())

    def v_parts(o):
        for k in o:
            assert torch.equal(_bits(o[k]), _bits(res[k])), k

    run_checked(two_parts, outs, bins, ws, v_parts)


# ------------------------------------------------------------------------------------------------ normalisation
def _norm_desc(n, hw, c, z_stride):
    from boxsegliver_amd._abi import NormDesc
    return NormDesc(n, hw, c, 0, z_stride, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0)


class _Unit(object):
    """One batch-norm + ReLU unit: y [N, H, W, C] and the float64 reference of z = relu(bn(y)) and its backward."""

    def __init__(self, n=2, h=8, w=12, c=64, seed=5):
        g = _gen(seed)
        self.n, self.h, self.w, self.c = n, h, w, c
        self.y = torch.randn((n, h, w, c), generator=g, device="cuda") * 1.5 + 0.3
        self.gamma = torch.rand(c, generator=g, device="cuda") + 0.5
        self.beta = torch.randn(c, generator=g, device="cuda") * 0.2
        y64 = self.y.double()
        self.mean = y64.mean((0, 1, 2))
        self.var = y64.var((0, 1, 2), unbiased=False)
        self.rstd = 1.0 / torch.sqrt(self.var + 1e-3)
        self.scale = self.gamma.double() * self.rstd
        self.shift = self.beta.double() - self.mean * self.scale
        self.f32 = {k: getattr(self, k).float() for k in ("mean", "rstd", "scale", "shift")}

    def z(self, y64):
        mu = y64.mean((0, 1, 2))
        rs = 1.0 / torch.sqrt(y64.var((0, 1, 2), unbiased=False) + 1e-3)
        return torch.relu(self.gamma.double() * (y64 - mu) * rs + self.beta.double())

    def backward(self, dz):
        y64 = self.y.double().requires_grad_(True)
        g64, b64 = self.gamma.double().requires_grad_(True), self.beta.double().requires_grad_(True)
        mu = y64.mean((0, 1, 2))
        rs = 1.0 / torch.sqrt(y64.var((0, 1, 2), unbiased=False) + 1e-3)
        z = torch.relu(g64 * (y64 - mu) * rs + b64)
        return torch.autograd.grad(z, (y64, g64, b64), dz)


def test_norm_finalize_edges(ops):
    u = _Unit()
    n, c = u.n, u.c
    d = _norm_desc(n, u.h * u.w, c, c)
    rows = 6                     # per-tile partial rows: split the pixels into 6 groups
    yr = u.y.reshape(rows, -1, c)
    stats = torch.stack((yr.sum(1), (yr * yr).sum(1)))
    g_in = {k: guarded_input(t) for k, t in (("stats", stats), ("gamma", u.gamma), ("beta", u.beta))}
    mm0 = torch.randn(c, device="cuda", generator=_gen(1))
    mv0 = torch.rand(c, device="cuda", generator=_gen(2)) + 0.5
    inout = {"moving_mean": guarded_input(mm0), "moving_var": guarded_input(mv0)}
    outs = {k: guarded((1, c)) for k in ("mean", "rstd", "scale", "shift")}
    ws = lib().unetk_norm_finalize_ws_bytes(ctypes.byref(d), rows)
    decay = 0.999
    m = u.y.numel() // c

    def launch(wsp, nb):
        return lib().unetk_norm_finalize(ctypes.byref(d), P(g_in["stats"]), rows, P(g_in["gamma"]), P(g_in["beta"]),
                                         ctypes.c_float(1e-3), ctypes.c_float(decay), 1, P(inout["moving_mean"]),
                                         P(inout["moving_var"]), P(outs["mean"]), P(outs["rstd"]), P(outs["scale"]),
                                         P(outs["shift"]), wsp, nb, stream())

    def verify(o):
        for k, ref in (("mean", u.mean), ("rstd", u.rstd), ("scale", u.scale), ("shift", u.shift)):
            torch.testing.assert_close(o[k][0].double(), ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(inout["moving_mean"].view.double(), mm0.double() * decay + u.mean * (1 - decay),
                                   rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(inout["moving_var"].view.double(),
                                   mv0.double() * decay + u.var * m / (m - 1) * (1 - decay), rtol=1e-5, atol=1e-6)

    run_checked(launch, outs, g_in, ws, verify, inout=inout, kernels=("norm_reduce_finalize_kernel(",))


@pytest.mark.parametrize("flagged", [False, True], ids=["one_pass", "refined"])
def test_norm_finalize_y_edges(ops, flagged):
    """unetk_norm_finalize_y: y = NULL is unetk_norm_finalize bit for bit; y of channels at mean / std about 27 takes the
    second pass over y (the one-pass variance is off by more than the keep tolerance there)."""
    u = _Unit()
    n, c = u.n, u.c
    d = _norm_desc(n, u.h * u.w, c, c)
    rows = 6
    y = u.y + 40.0 if flagged else u.y
    yr = y.reshape(rows, -1, c)
    stats = torch.stack((yr.sum(1), (yr * yr).sum(1)))
    g_in = {k: guarded_input(t) for k, t in (("stats", stats), ("gamma", u.gamma), ("beta", u.beta))}
    if flagged:
        g_in["y"] = guarded_input(y)
    mm0 = torch.randn(c, device="cuda", generator=_gen(1))
    mv0 = torch.rand(c, device="cuda", generator=_gen(2)) + 0.5
    inout = {"moving_mean": guarded_input(mm0), "moving_var": guarded_input(mv0)}
    outs = {k: guarded((1, c)) for k in ("mean", "rstd", "scale", "shift")}
    ws = lib().unetk_norm_finalize_ws_bytes(ctypes.byref(d), rows)
    decay = 0.999
    m = y.numel() // c
    y64 = y.double()
    mean = y64.mean((0, 1, 2))
    var = y64.var((0, 1, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-3)
    scale = u.gamma.double() * rstd
    shift = u.beta.double() - mean * scale

    def args(fn, wsp, nb, yp):
        head = (ctypes.byref(d), P(g_in["stats"]), rows) + ((yp,) if fn == "y" else ())
        return head + (P(g_in["gamma"]), P(g_in["beta"]), ctypes.c_float(1e-3), ctypes.c_float(decay), 1,
                       P(inout["moving_mean"]), P(inout["moving_var"]), P(outs["mean"]), P(outs["rstd"]),
                       P(outs["scale"]), P(outs["shift"]), wsp, nb, stream())

    def launch(wsp, nb):
        return lib().unetk_norm_finalize_y(*args("y", wsp, nb, P(g_in.get("y"))))

    def verify(o):
        for k, ref in (("mean", mean), ("rstd", rstd), ("scale", scale), ("shift", shift)):
            torch.testing.assert_close(o[k][0].double(), ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(inout["moving_mean"].view.double(), mm0.double() * decay + mean * (1 - decay),
                                   rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(inout["moving_var"].view.double(),
                                   mv0.double() * decay + var * m / (m - 1) * (1 - decay), rtol=1e-5, atol=1e-6)

    run_checked(launch, outs, g_in, ws, verify, inout=inout,
                kernels=("norm_reduce_finalize_kernel(",) + (("norm_refine_kernel(",) if flagged else ()),
                absent=() if flagged else ("norm_refine_kernel(",))
    if not flagged:      # NULL activations: the results of unetk_norm_finalize, bit for bit
        wsb = GuardedWorkspace(ws)
        got = {}
        for fn in ("y", "plain"):
            for o in list(outs.values()) + list(inout.values()):
                o.reset()
            f = lib().unetk_norm_finalize_y if fn == "y" else lib().unetk_norm_finalize
            assert f(*args(fn, P(wsb.ptr()), wsb.nbytes, None)) == 0
            torch.cuda.synchronize()
            got[fn] = [_bits(o.view.clone()) for o in list(outs.values()) + list(inout.values())]
        assert all(torch.equal(a, b) for a, b in zip(got["y"], got["plain"]))


def test_norm_apply_relu_strided_and_pooled_edges(ops):
    u = _Unit()
    n, h, w, c = u.n, u.h, u.w, u.c
    zs = c + 64
    d = _norm_desc(n, h * w, c, zs)
    z_ref = torch.relu(u.y.double() * u.scale + u.shift)
    gy = guarded_input(u.y)
    gsc, gsh = guarded_input(u.f32["scale"]), guarded_input(u.f32["shift"])
    ins = {"y": gy, "scale": gsc, "shift": gsh}
    gz = guarded((n, h, w, c), pixel_stride=zs, coff=32)
    run_checked(lambda wsp, nb: lib().unetk_norm_apply_relu(ctypes.byref(d), P(gy), P(gsc), P(gsh), None, None, None, None,
                                                            P(gz), stream()),
                {"z": gz}, ins, 0, lambda o: _lt(rel(o["z"], z_ref), 1e-5), kernels=("norm_apply_relu_kernel<0, false, false, float>",))
    gp = guarded((n, h // 2, w // 2, c))

    def v_pool(o):
        assert rel(o["z"], z_ref) < 1e-5
        assert torch.equal(o["pooled"], o["z"].reshape(n, h // 2, 2, w // 2, 2, c).amax((2, 4)))

    run_checked(lambda wsp, nb: lib().unetk_norm_apply_relu_pool(ctypes.byref(d), w, P(gy), P(gsc), P(gsh), P(gz), P(gp),
                                                                 stream()),
                {"z": gz, "pooled": gp}, ins, 0, v_pool, kernels=("norm_apply_relu_pool_kernel<float>",))


NBR_REDUCE = "norm_bwd_reduce_kernel<0, false, false, float, false>"
NBR_APPLY = "norm_bwd_apply_kernel<0, false, false, float>"


def test_norm_relu_bwd_edges(ops):
    """unetk_norm_relu_bwd with dz a concat slice, and unetk_norm_relu_bwd_pre with the reduction given as partials."""
    u = _Unit(seed=9)
    n, h, w, c = u.n, u.h, u.w, u.c
    dzs = c + 64
    d = _norm_desc(n, h * w, c, c)
    dz = torch.randn((n, h, w, c), generator=_gen(4), device="cuda")
    dy_ref, dg_ref, db_ref = u.backward(dz.double())
    gy, gdz = guarded_input(u.y), guarded_input(dz, dzs, 32)
    par = {k: guarded_input(t) for k, t in u.f32.items()}
    ins = dict(par, y=gy, dz=gdz)
    ws = lib().unetk_norm_bwd_ws_bytes(ctypes.byref(d))

    def outs():
        return {"dy": guarded((n, h, w, c)), "dgamma": guarded((c,)), "dbeta": guarded((c,))}

    o1 = outs()

    def verify(o):
        assert rel(o["dy"], dy_ref) < 2e-5
        assert rel(o["dgamma"], dg_ref) < 2e-5
        assert rel(o["dbeta"], db_ref) < 2e-5

    def bwd(wsp, nb):
        return lib().unetk_norm_relu_bwd(ctypes.byref(d), P(gy), P(gdz), dzs, P(par["scale"]), P(par["shift"]),
                                         P(par["mean"]), P(par["rstd"]), None, None, None, None, P(o1["dy"]),
                                         P(o1["dgamma"]), P(o1["dbeta"]), None, None, None, wsp, nb, stream())

    run_checked(bwd, o1, ins, ws, verify, kernels=(NBR_REDUCE, NBR_APPLY))

    # the reduction as partials [2][rows][C]: sum du and sum du * xhat over 4 row groups of the pixels
    y64 = u.y.double()
    du = dz.double() * ((y64 * u.f32["scale"].double() + u.f32["shift"].double()) > 0)
    xhat = (y64 - u.f32["mean"].double()) * u.f32["rstd"].double()
    pre_rows = 4
    pre = torch.stack((du.reshape(pre_rows, -1, c).sum(1), (du * xhat).reshape(pre_rows, -1, c).sum(1))).float()
    gpre = guarded_input(pre)
    o2 = outs()

    def bwd_pre(wsp, nb):
        return lib().unetk_norm_relu_bwd_pre(ctypes.byref(d), P(gy), P(gdz), dzs, P(par["scale"]), P(par["shift"]),
                                             P(par["mean"]), P(par["rstd"]), None, None, None, None, P(o2["dy"]),
                                             P(o2["dgamma"]), P(o2["dbeta"]), None, None, None, P(gpre), pre_rows, wsp, nb,
                                             stream())

    run_checked(bwd_pre, o2, dict(ins, pre=gpre), ws, verify, kernels=(NBR_APPLY,),
                absent=("norm_bwd_reduce_kernel",))


def test_norm_relu_bwd_pool_edges(ops):
    """The encoder's second unit: dz = dskip (a concat-gradient slice) + the pooled gradient routed to the first maximum."""
    u = _Unit(seed=13)
    n, h, w, c = u.n, u.h, u.w, u.c
    dss = c + 64
    d = _norm_desc(n, h * w, c, c)
    g = _gen(6)
    dskip = torch.randn((n, h, w, c), generator=g, device="cuda")
    dp = torch.randn((n, h // 2, w // 2, c), generator=g, device="cuda")
    z = torch.relu(u.y.double() * u.f32["scale"].double() + u.f32["shift"].double())
    win = z.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    first = win.argmax(-1)                         # first maximum in scan order
    route = torch.nn.functional.one_hot(first, 4).double() * dp.double()[..., None]
    route = route.reshape(n, h // 2, w // 2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)
    dy_ref, dg_ref, db_ref = u.backward(dskip.double() + route)
    gy, gds, gdp = guarded_input(u.y), guarded_input(dskip, dss, 32), guarded_input(dp)
    par = {k: guarded_input(t) for k, t in u.f32.items()}
    outs = {"dy": guarded((n, h, w, c)), "dgamma": guarded((c,)), "dbeta": guarded((c,))}
    ws = lib().unetk_norm_bwd_ws_bytes(ctypes.byref(d))

    def launch(wsp, nb):
        return lib().unetk_norm_relu_bwd_pool(ctypes.byref(d), w, P(gy), P(gds), dss, P(gdp), P(par["scale"]),
                                              P(par["shift"]), P(par["mean"]), P(par["rstd"]), P(outs["dy"]),
                                              P(outs["dgamma"]), P(outs["dbeta"]), wsp, nb, stream())

    def verify(o):
        assert rel(o["dy"], dy_ref) < 2e-5
        assert rel(o["dgamma"], dg_ref) < 2e-5
        assert rel(o["dbeta"], db_ref) < 2e-5

    run_checked(launch, outs, dict(par, y=gy, dskip=gds, dp=gdp), ws, verify,
                kernels=("norm_bwd_reduce_pool_kernel<float>", "norm_bwd_apply_pool_kernel<float>"))


# ------------------------------------------------------------------------------------------------ loss head
HEAD_ROWS = [
    # name, N, HW, C, ncls, weight mode
    ("c64_k3", 2, 1025, 64, 3, "numerical"),
    ("c32_k2", 3, 255, 32, 2, "pixelmap"),
    ("c8_k8_ragged", 2, 7, 8, 8, "proportion"),              # HW not a multiple of the 2 lanes per pixel
    ("c8_k3_tmp", 2, 140000, 8, 3, "none"),                  # 1094 backward blocks: dw and db both go through `tmp`
]


@pytest.mark.parametrize("storage", ["fp32", "bf16s"])
@pytest.mark.parametrize("row", HEAD_ROWS, ids=[r[0] for r in HEAD_ROWS])
def test_head_fwd_bwd_edges(ops, row, storage):
    """unetk_head_fwd + unetk_head_bwd on one shared workspace of exactly unetk_head_ws_bytes (hist, wn, part, pw, pb, tmp);
    result holds exactly unetk_head_result_floats; one byte less of workspace is refused before anything is written."""
    import test_gpu_head as th
    from boxsegliver_amd import _abi
    _, n, hw, c, ncls, mode = row
    bf = storage == "bf16s"
    sdt = torch.bfloat16 if bf else torch.float32
    case = th._case("guard_" + row[0], n, hw, c, ncls, mode, None, storage="bf16" if bf else "fp32")
    z, w, b, labels, pixel_w = th.make_inputs(case)
    ref = th.ref_of(case, (z, w, b, labels, pixel_w))
    d = th.desc_of(ops, case)
    d.storage = _abi.BF16S if bf else _abi.FP32
    npix = n * hw
    nres, nws = lib().unetk_head_result_floats(ctypes.byref(d)), lib().unetk_head_ws_bytes(ctypes.byref(d))
    assert nres == 3 + n * (ncls - 1) * 4 + n * 2 and nws == th.head_paths(n, hw, c, ncls)["ws_bytes"]
    assert (th.head_paths(n, hw, c, ncls)["nblk"] > 1024) == (row[0] == "c8_k3_tmp")
    ins = {"z": guarded_input(z.reshape(npix, c).cuda(), dtype=sdt), "w": guarded_input(w.cuda()),
           "b": guarded_input(b.cuda()), "labels": guarded_input(labels.reshape(npix, 1).cuda().view(torch.float32))}
    if pixel_w is not None:
        ins["pixel_w"] = guarded_input(pixel_w.reshape(npix, 1).cuda())
    outs = {"logits": guarded((npix, ncls)), "probs": guarded((npix, ncls)), "result": guarded((nres,)),
            "dz": guarded((npix, c), sdt), "dw": guarded((c, ncls)), "db": guarded((ncls,))}
    scales = torch.tensor([0.5, 2.0], device="cuda")
    xs, ds = 0.7, 0.3

    def fwd(wsp, nb):
        return lib().unetk_head_fwd(ctypes.byref(d), P(ins["z"]), P(ins["w"]), P(ins["b"]), P(ins["labels"]),
                                    P(ins.get("pixel_w")), P(outs["logits"]), P(outs["probs"]), P(outs["result"]), wsp, nb,
                                    stream())

    def bwd(wsp, nb):
        return lib().unetk_head_bwd(ctypes.byref(d), P(ins["z"]), P(ins["w"]), P(ins["labels"]), P(ins.get("pixel_w")),
                                    P(outs["logits"]), P(outs["result"]), xs, ds, P(scales), P(outs["dz"]), P(outs["dw"]),
                                    P(outs["db"]), wsp, nb, stream())

    def launch(wsp, nb):
        return fwd(wsp, nb) or bwd(wsp, nb)

    exp = [xs * 0.5 * (gx if gx is not None else 0.0) + ds * 2.0 * gd for gx, gd in zip(ref["gx"], ref["gd"])]

    def verify(o):
        res = o["result"].double().cpu()
        head3, sums, iu = th.split_result(res, n, ncls)
        assert rel(o["logits"].reshape(n, hw, ncls), ref["logits"].to("cuda")) < 3e-6
        assert (o["probs"].reshape(n, hw, ncls).double() - ref["probs"].to("cuda")).abs().max().item() < 2e-6
        assert abs(head3[0].item() - ref["xent"]) < 2e-5 * max(1.0, abs(ref["xent"]))
        assert abs(head3[1].item() - ref["dice"]) < 2e-5
        assert head3[2].item() == ref["present"]
        assert ((iu - ref["iu"].cpu()).abs() / ref["iu"].cpu().abs().clamp_min(1.0)).max().item() < 2e-5
        th.check_counts(sums, ref)
        if bf:
            _stored_ok(o["dz"].reshape(n, hw, c), exp[0].to("cuda"), flips=5e-3)
        else:
            assert rel(o["dz"].reshape(n, hw, c), exp[0].to("cuda")) < 2e-5
        assert rel(o["dw"], exp[1].to("cuda")) < 2e-5
        assert rel(o["db"], exp[2].to("cuda")) < 2e-5

    kernels = ("head_fwd_kernel", "head_finalize_kernel", "head_bwd_kernel")
    run_checked(launch, outs, ins, nws, verify, kernels=kernels + (("rows_reduce_l1_kernel",) if row[0] == "c8_k3_tmp" else ()))
    # one byte less: UNETK_E_WORKSPACE from both entry points, nothing written anywhere
    short = GuardedWorkspace(nws - 1)
    short.fill(0x5F)
    before = short.buf.clone()
    for o in outs.values():
        o.reset()
    for call in (fwd, bwd):
        rc = call(P(short.ptr()), short.nbytes)
        torch.cuda.synchronize()
        assert rc == E_WORKSPACE, rc
        assert all(o.changed_anywhere() == 0 for o in outs.values()) and torch.equal(short.buf, before)
    assert all(i.changed_anywhere() == 0 for i in ins.values())


@pytest.mark.parametrize("npix", [1000, 4096 * 256 + 77], ids=["ragged_block", "past_grid_cap"])
def test_head_predict_edges(ops, npix):
    """unetk_head_predict: argmax and the thresholded masks (uint8; 0xA5 is no valid value of either) inside guards."""
    ncls, guard = 3, 256 << 10
    probs = torch.softmax(2.0 * torch.randn((npix, ncls), generator=_gen(npix % 97), device="cuda"), -1)
    gp = guarded_input(probs)
    bufs = {"argmax": torch.full((2 * guard + npix,), 0xA5, dtype=torch.uint8, device="cuda"),
            "preds": torch.full((2 * guard + (ncls - 1) * npix,), 0xA5, dtype=torch.uint8, device="cuda")}
    rc = lib().unetk_head_predict(P(gp), npix, ncls, P(bufs["argmax"].data_ptr() + guard), P(bufs["preds"].data_ptr() + guard),
                                  stream())
    torch.cuda.synchronize()
    assert rc == 0 and gp.changed_anywhere() == 0
    for name, t in bufs.items():
        assert bool((t[:guard] == 0xA5).all()) and bool((t[-guard:] == 0xA5).all()), name
    assert torch.equal(bufs["argmax"][guard:-guard], probs.argmax(-1).to(torch.uint8))
    assert torch.equal(bufs["preds"][guard:-guard].reshape(ncls - 1, npix), (probs[:, 1:] > 0.5).t().to(torch.uint8))
