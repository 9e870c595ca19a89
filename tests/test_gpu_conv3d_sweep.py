"""The 3-D conv composition (csrc/conv3d.hip) over the extent grid of tests/conv3d_sweep_cases.py, exactly.

One item per (kernel depth, stride) family and channel pair.  Every case of the item runs unetk_conv3d_fwd with statistics,
unetk_conv3d_dgrad and unetk_conv3d_wgrad straight through the C ABI: outputs in guarded buffers (tests/guardbuf.py: dense, or
channel slices of buffers 32 channels wider), the workspace exactly the queried size with a sentinel guard behind it, each
call traced.  The inputs make fp32 arithmetic exact in any summation order (test_conv3d_sweep_host.py checks the regime of every
case), so there is no tolerance anywhere:

  eighths  y, dx, dw bit-equal to the float64 reference; no sentinel left inside a view, nothing changed outside one, the
           workspace guard intact, the read-only inputs unchanged, dw bit-equal on a second call;
  sparse   (forward) y bit-equal; the per-sample sums of the statistic partials equal sum y and sum y^2 of the reference; the
           partials are the unetk_conv3d_stat_rows(d) rows of a guarded [2][rows][Cout] buffer, every one written, none beyond;
  both     the branch decoded from each op's launch trace is the one the restatement of the dispatch names.

A refusal by the library is a failure.  An item reports every failing case with the launches of its three ops, and prints
branch -> number of cases; the last test asserts that the items together reached every branch, the input gradient's dilated
fallback in all three stride-2 families at both depth parities.
"""
import collections
import ctypes

import pytest
import torch

import conv3d_sweep_cases as S
from guardbuf import SENTINEL, GuardedWorkspace, guarded, guarded_input
from oracle import tf_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


def P(x):
    if x is None:
        return None
    return ctypes.c_void_p(x if isinstance(x, int) else (x.ptr() if hasattr(x, "ptr") else x.data_ptr()))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _trace(ops, fn):
    """(return code, launches in order) -- names as test_gpu_ops3d._trace writes them."""
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        rc = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    launches = []
    for name in ops.profile_read()[1]:
        name = name.replace(" ", "").replace("(anonymousnamespace)::", "").split("(")[0]
        launches.append(name[4:] if name.startswith("void") else name)
    return rc, launches


def reference(c, kind, backward):
    x, w, dy = S.make_inputs(c, kind)
    if not backward:
        with torch.no_grad():
            return x, w, dy, tf_ops.conv_nd_same(x, w, stride=c.stride), None, None
    x.requires_grad_(True)
    w.requires_grad_(True)
    y = tf_ops.conv_nd_same(x, w, stride=c.stride)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    return x.detach(), w.detach(), dy, y.detach(), dx, dw


def _flags(out, ws, ins):
    """Device-side edge checks of one call, one transfer: sentinels left inside the output view, elements changed outside it,
    workspace guard intact, read-only inputs unchanged."""
    bits, snap = out.bits(), out.bits(out.snap)
    f = [((bits == SENTINEL[out.dtype]) & out.mask).sum(), ((bits != snap) & ~out.mask).sum()]
    f += [(i.bits() != i.bits(i.snap)).sum() for i in ins]
    unwritten, outside = int(f[0]), int(f[1])
    errs = []
    if unwritten:
        errs.append("{} elements never written".format(unwritten))
    if outside:
        errs.append("{} elements outside the view changed".format(outside))
    if not ws.guard_intact():
        errs.append("workspace used beyond its {} bytes".format(ws.nbytes))
    if any(int(v) for v in f[2:]):
        errs.append("a read-only input changed")
    return errs


def _neq(got, ref64):
    """Number of elements of a device fp32 tensor that are not bit-equal to the float64 reference (which is exact in fp32;
    -0.0 counts as 0.0)."""
    return int((got.double().cpu() != ref64).sum()) + int(torch.isnan(got).sum())


def run_case(ops, c):
    """-> (list of error strings, (fwd launches, dgrad launches, wgrad launches))."""
    L = lib()
    from boxsegliver_amd._abi import Conv3dDesc
    errs = []
    xs = c.cin + (S.SLICE_EXTRA if c.sliced else 0)
    ys = c.cout + (S.SLICE_EXTRA if c.sliced else 0)
    d = Conv3dDesc(c.n, c.d, c.h, c.w, c.cin, c.cout, c.kd, c.stride[0], c.stride[1], xs, ys)
    pd = ctypes.byref(d)
    want, g = S.branch(c), S.geo(c)
    do, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = L.unetk_conv3d_out_dims(pd, ctypes.byref(do), ctypes.byref(ho), ctypes.byref(wo))
    if rc != 0 or (do.value, ho.value, wo.value) != (g.do, g.ho, g.wo):
        return ["out_dims rc {} -> {}".format(rc, (do.value, ho.value, wo.value))], ([], [], [])
    rows, ws_bytes = L.unetk_conv3d_stat_rows(pd), L.unetk_conv3d_ws_bytes(pd)
    if rows <= 0 or rows % c.n:
        return ["stat_rows {}".format(rows)], ([], [], [])
    yshape = S.out_shape(c)
    traces = [[], [], []]

    def decoded(i, op, launches):
        traces[i] = launches
        got = S.decode(c, op, launches)
        if got != want[i]:
            errs.append("{}: the launches show `{}`, the restatement says `{}`".format(op, got, want[i]))
        return got

    def forward(kind):
        x, w, dy, y_ref, dx_ref, dw_ref = reference(c, kind, backward=kind == "eighths")
        wd = w.float().cuda()
        wp_f, wp_d = torch.empty(wd.numel(), device="cuda"), torch.empty(wd.numel(), device="cuda")
        if L.unetk_conv3d_pack(P(wd), c.kd, c.cin, c.cout, P(wp_f), P(wp_d), stream()) != 0:
            errs.append(kind + ": pack refused")
            return None
        gx, gw = guarded_input(x.float().cuda(), xs, c.xoff), guarded_input(wp_f.reshape(-1, 4))
        gy, gs = guarded(yshape, pixel_stride=ys, coff=c.yoff), guarded((2, rows, c.cout))
        ws = GuardedWorkspace(ws_bytes)
        ws.fill(0xFF)                       # scratch is read only after it is written: NaN otherwise
        rc, t = _trace(ops, lambda: L.unetk_conv3d_fwd(pd, P(gx), P(gw), P(gy), P(gs), P(ws.ptr()), ws.nbytes, stream()))
        decoded(0, "fwd", t)
        if rc != 0:
            errs.append("{} fwd: return code {}".format(kind, rc))
            return None
        errs.extend("{} fwd y: {}".format(kind, e) for e in _flags(gy, ws, (gx, gw)))
        errs.extend("{} fwd stats: {}".format(kind, e) for e in _flags(gs, ws, ()))
        bad = _neq(gy.view, y_ref)
        if bad:
            errs.append("{} fwd: {} of {} elements of y differ from float64".format(kind, bad, y_ref.numel()))
        if kind == "sparse":
            per = gs.view.double().cpu().reshape(2, c.n, rows // c.n, c.cout).sum(2)
            r = y_ref.reshape(c.n, -1, c.cout)
            if not torch.equal(per[0], r.sum(1)):
                errs.append("sparse fwd: the statistic partials do not sum to sum y")
            if not torch.equal(per[1], (r * r).sum(1)):
                errs.append("sparse fwd: the statistic partials do not sum to sum y^2")
        return x, dy, dx_ref, dw_ref, gx, wp_d

    got = forward("eighths")
    if got is not None:
        x, dy, dx_ref, dw_ref, gx, wp_d = got
        gdy, gwd = guarded_input(dy.float().cuda(), ys, c.yoff), guarded_input(wp_d.reshape(-1, 4))
        gdx = guarded((c.n, c.d, c.h, c.w, c.cin), pixel_stride=xs, coff=c.xoff)
        ws = GuardedWorkspace(ws_bytes)
        ws.fill(0xFF)
        rc, t = _trace(ops, lambda: L.unetk_conv3d_dgrad(pd, P(gdy), P(gwd), P(gdx), P(ws.ptr()), ws.nbytes, stream()))
        decoded(1, "dgrad", t)
        if rc != 0:
            errs.append("dgrad: return code {}".format(rc))
        else:
            errs.extend("dgrad dx: {}".format(e) for e in _flags(gdx, ws, (gdy, gwd)))
            bad = _neq(gdx.view, dx_ref)
            if bad:
                errs.append("dgrad: {} of {} elements of dx differ from float64".format(bad, dx_ref.numel()))
        gdw = guarded((c.kd, 3, 3, c.cin, c.cout))
        ws = GuardedWorkspace(ws_bytes)
        ws.fill(0xFF)
        rc, t = _trace(ops, lambda: L.unetk_conv3d_wgrad(pd, P(gx), P(gdy), P(gdw), P(ws.ptr()), ws.nbytes, stream()))
        decoded(2, "wgrad", t)
        if rc != 0:
            errs.append("wgrad: return code {}".format(rc))
        else:
            errs.extend("wgrad dw: {}".format(e) for e in _flags(gdw, ws, (gx, gdy)))
            bad = _neq(gdw.view, dw_ref)
            if bad:
                errs.append("wgrad: {} of {} elements of dw differ from float64".format(bad, dw_ref.numel()))
            first = gdw.view.clone()
            gdw.reset()
            ws.fill(0x5F)
            rc = L.unetk_conv3d_wgrad(pd, P(gx), P(gdy), P(gdw), P(ws.ptr()), ws.nbytes, stream())
            if rc != 0 or not torch.equal(gdw.view.view(torch.int32), first.view(torch.int32)):
                errs.append("wgrad: the second call (rc {}) is not bit-equal to the first".format(rc))
    eighths_traces = tuple(traces)
    forward("sparse")
    if traces[0] != eighths_traces[0]:
        errs.append("fwd: the sparse inputs ran other launches than the eighths: {}".format(traces[0]))
    return errs, eighths_traces


_RESULTS = {}


def run_item(ops, item):
    """-> (failure texts, branch -> cases, depth parities at which the dilated input-gradient fallback ran); run once."""
    if item not in _RESULTS:
        failed, count, dilated = [], collections.Counter(), set()
        for c in S.cases(*item):
            errs, traces = run_case(ops, c)
            for i, op in enumerate(("fwd", "dgrad", "wgrad")):
                b = S.decode(c, op, traces[i])
                if not b.startswith("?"):
                    count[b] += 1
                    if b == S.D_DILATED:
                        dilated.add(c.d % 2)
            if errs:
                failed.append("{}\n    {}\n    fwd {}\n    dgrad {}\n    wgrad {}".format(S.case_id(c), "\n    ".join(errs), *traces))
        _RESULTS[item] = failed, count, dilated
    return _RESULTS[item]


def _table(title, count):
    print("\n{}: branch -> cases".format(title))
    for b in S.BRANCHES:
        if count[b]:
            print("  {:36s} {}".format(b, count[b]))


@pytest.mark.parametrize("item", S.ITEMS, ids=[S.item_id(i) for i in S.ITEMS])
def test_conv3d_sweep(ops, item):
    failed, count, _ = run_item(ops, item)
    _table(S.item_id(item), count)
    assert not failed, "{} of {} cases failed:\n{}".format(len(failed), len(S.cases(*item)), "\n".join(failed))


def test_conv3d_sweep_reached_every_branch(ops):
    """Over all items (those the run has not done yet are run here)."""
    reached, dilated_at = collections.Counter(), set()
    for item in S.ITEMS:
        _, count, dilated = run_item(ops, item)
        reached.update(count)
        dilated_at |= {(item[0], par) for par in dilated}
    _table("all items", reached)
    missing = [b for b in S.BRANCHES if reached[b] < 8]
    assert not missing, "branches reached by fewer than 8 cases: {}".format({b: reached[b] for b in missing})
    want = {(f, par) for f in S.STRIDE2_FAMILIES for par in (0, 1)}
    assert dilated_at == want, "dilated input-gradient fallback missing at {}".format(sorted(want - dilated_at))
