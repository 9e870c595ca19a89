"""The pool, image-feature, context-branch and boundary-weight kernels (csrc/pool.hip, fc.hip, conv1d.hip, weights.hip) on every
path, through the C ABI (table and float64 restatements: tests/small_ops_cases.py).

Every call runs in tests/guardbuf.py buffers: inputs poisoned around the data and bit-equal afterwards, outputs sentinel-filled
(nothing outside the view changes, no sentinel is left inside), the dpre_ws buffers and the boundary workspace GuardedWorkspaces of
exactly the documented / queried size that start as NaN patterns.  Every call asserts its launch trace in order and runs twice,
bit-equal.  One row per family also goes through the ops.py wrapper (the autograd ops: compared with the ABI call bit for bit).

Exact tier: results equal float64 bit for bit (bf16 storage: float64 rounded once; -0.0 == +0.0, as a pooled zero may carry either
sign).  spatial_mean_fwd divides once: float32(float64(sum) / HW).  spatial_mean_bwd multiplies by float32(1 / HW): float64 where
HW is a power of two, else the float32 restatement of exactly those two roundings.  Bound tier on the same rows: FC / conv1d
rel < 1e-5, pools and image gradients bit-equal, sobel rel < 1e-6, avg-pool atol 1e-7 on uniform inputs (the bounds of the existing
tests of these kernels); spatial_mean_fwd 4 x the measured error of the float32 restatement of its summation order
(small_ops_cases.SPATIAL_MEAN_REL); flip_axpy two fp32 roundings; guide_moments one fp32 rounding of a float64 mean.  The boundary
map compares at rtol 2e-6 in every tier (expf and the normalising sum are not exact); its two runs are bit-equal.  The max-pool cap
rows (134 MB of fp32 payload) run once: fp32 forward and backward, bf16 backward only, exact tier.
"""
import ctypes

import numpy as np
import pytest
import torch

import guardbuf
import small_ops_cases as T

pytestmark = pytest.mark.gpu

E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16
WRAP = {"mp_blocks5", "ap_c3", "ig_c3", "sb_c3_last", "fl_11_acc", "gm_ps_g4_p257", "sm_hw5_c65", "fc_n257_keep4", "c1_k3_l37", "p1_l7",
        "bw_single_between"}


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    lib()
    return _ops


def _p(t):
    if t is None:
        return None
    return ctypes.c_void_p(t if isinstance(t, int) else (t.ptr() if hasattr(t, "ptr") else t.data_ptr()))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _norm(name):
    return name.replace(" ", "").replace("(anonymousnamespace)::", "")


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return out, [_norm(n) for n in ops.profile_read()[1]]


def _assert_trace(names, expect, what):
    assert len(names) == len(expect) and all(e in g for e, g in zip(expect, names)), "{}: traced {} expected {}".format(what, names, expect)


def _dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dtype)


def _host(t):
    return t.float().cpu().numpy().astype(np.float64)


def _sd(storage):
    return BF16 if storage == T.BF16S else F32


def _tn(storage):
    return "unsignedshort" if storage == T.BF16S else "float"


def _equal(got_t, want, what):
    """Value equality with float64 (-0.0 == +0.0; no NaN on either side).  The largest rows compare on the device: their expected
    values are fp32- / bf16-representable (asserted in tests/test_small_ops_host.py), so the upload rounds nothing."""
    if want.size > 1 << 22:
        w32 = np.ascontiguousarray(want, dtype=np.float32)
        assert np.array_equal(w32, want), what
        bad = got_t.float() != torch.from_numpy(w32).cuda().reshape(got_t.shape)
        assert not bool(bad.any()), "{}: {} of {} elements differ from float64".format(what, int(bad.sum()), want.size)
        return
    assert np.any(want != 0), what + ": the expected output is identically zero"
    got = _host(got_t).reshape(np.shape(want))
    bad = got != want
    assert not bad.any(), "{}: {} of {} elements differ from float64, first at {}".format(what, int(bad.sum()), got.size,
                                                                                        np.argwhere(bad)[:3].tolist())


def _rel(got_t, want, what, bound):
    got = _host(got_t).reshape(np.shape(want))
    assert np.isfinite(got).all() and np.any(want != 0), what
    e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    print(what, "rel err", e, "bound", bound)
    assert e < bound, (what, e)


class Run(object):
    """The guarded buffers of one row and its calls: trace, guards, a second bit-equal run."""

    def __init__(self, ops):
        self.ops, self.ins, self.outs, self.wss = ops, [], [], []

    def i(self, a, dtype=F32, stride=None, coff=0):
        g = guardbuf.guarded_input(_dev(a, dtype), pixel_stride=stride, coff=coff)
        self.ins.append(g)
        return g

    def labels(self, lab):
        g = guardbuf.guarded_input(torch.from_numpy(lab).cuda().view(F32))           # int32 bits in an fp32 guarded buffer
        self.ins.append(g)
        return g

    def o(self, shape, dtype=F32, stride=None, coff=0, init=None):
        g = guardbuf.guarded(shape, dtype, stride, coff) if init is None else guardbuf.guarded_input(_dev(init, dtype))
        self.outs.append(g)
        return g

    def ws(self, nbytes):
        w = guardbuf.GuardedWorkspace(nbytes)
        self.wss.append(w)
        return w

    def check(self, what, outs):
        for o in outs:
            assert o.check_untouched(), what + ": wrote outside an output view"
            assert o.unwritten() == 0, what + ": left output elements unwritten"
        for i in self.ins:
            assert i.changed_anywhere() == 0, what + ": changed an input"
        for w in self.wss:
            assert w.guard_intact(), what + ": wrote outside the workspace"

    def go(self, fn, expect, what, outs):
        for w in self.wss:
            w.fill(0xFF)                                         # NaN patterns: nothing may be read before it is written
        rc, names = _trace(self.ops, fn)
        assert rc == 0, (what, rc)
        _assert_trace(names, expect, what)
        self.check(what, outs)
        first = [o.bits().clone() for o in outs]
        for o in outs:
            o.reset()
        for w in self.wss:
            w.fill(0xFF)
        assert fn() == 0
        torch.cuda.synchronize()
        self.check(what + " (second run)", outs)
        for o, f in zip(outs, first):
            assert torch.equal(o.bits(), f), what + ": not bit-reproducible"


_CASES = {}


def _case(row, tier, storage=T.FP32S):
    """Inputs and the float64 reference, computed once per (row, tier, storage); the cap rows of the max-pool share one."""
    key = (row.id, tier, T.FP32S if row.p.get("cap") else storage)
    if key not in _CASES:
        a = T.make_inputs(row, tier, key[2])
        _CASES[key] = (a, T.reference(row, a, key[2]))
    return _CASES[key]


def _params(fam):
    out = []
    for r in T.rows(fam):
        for st in T.storages(r):
            for tier in ("exact", "gauss"):
                if tier == "exact" and not T.exact_tier(r):
                    continue
                if r.p.get("cap") and tier == "gauss":
                    continue                                     # 134 MB of payload: once (module docstring)
                name = r.id + ("-bf16s" if st == T.BF16S else "") + "-" + tier
                out.append(pytest.param(r.id, st, tier, id=name))
    return out


# ------------------------------------------------------------------ max-pool 2x2
@pytest.mark.parametrize("rid,storage,tier", _params("mp2"))
def test_maxpool2_row(ops, rid, storage, tier):
    row = T.BY_ID[rid]
    p = row.p
    n, h, w, c = p["n"], p["h"], p["w"], p["c"]
    a, ref = _case(row, tier, storage)
    sd, L = _sd(storage), lib()
    sfx = "_bf16" if storage == T.BF16S else ""
    fwd, bwd = getattr(L, "unetk_maxpool2_fwd" + sfx), getattr(L, "unetk_maxpool2_bwd" + sfx)
    xh = a["x"].copy()
    if h % 2:
        xh[:, h - 1] = guardbuf.POISON                           # VALID: the odd last row / column is never read
    if w % 2:
        xh[:, :, w - 1] = guardbuf.POISON
    r = Run(ops)
    x = r.i(xh, sd, p["xs"], p["xo"])
    even = h % 2 == 0 and w % 2 == 0
    if not (p["cap"] and storage == T.BF16S):
        pool = r.o((n, h // 2, w // 2, c), sd)
        r.go(lambda: fwd(_p(x), p["xs"], _p(pool), n, h, w, c, _stream()), ["maxpool2_fwd_kernel<%s>" % _tn(storage)], rid + " fwd", [pool])
        _equal(pool.view, T.store(ref["p"], storage), rid + " pooled")
        if rid in WRAP:
            assert torch.equal(ops.maxpool2_fwd(x.view), pool.view)
    if not even:
        return
    pin, dp = r.i(T.store(ref["p"], storage), sd), r.i(a["dp"], sd)
    add = r.i(a["add"], sd, p["ast"], p["ao"]) if p["add"] else None
    dx = r.o((n, h, w, c), sd)
    r.go(lambda: bwd(_p(x), p["xs"], _p(pin), _p(dp), _p(add), p["ast"], _p(dx), n, h, w, c, _stream()),
         ["maxpool2_bwd_kernel<%s>" % _tn(storage)], rid + " bwd", [dx])
    _equal(dx.view, T.store(ref["dx"], storage), rid + " dx")
    if rid in WRAP:
        assert torch.equal(ops.maxpool2_bwd(x.view, pin.view, dp.view, add=add.view if add else None), dx.view)
    if p["cap"] and storage == T.BF16S:
        _CASES.pop((rid, tier, T.FP32S))                        # the row's last test: let go of its 0.7 GB of float64


# ------------------------------------------------------------------ avg-pool, image gradients, sobel, flip, moments
@pytest.mark.parametrize("rid,storage,tier", _params("avg"))
def test_avgpool2_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    n, h, w, c = p["n"], p["h"], p["w"], p["c"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    x, out = r.i(a["x"]), r.o((n, h // 2, w // 2, c))
    r.go(lambda: lib().unetk_avgpool2_fwd(_p(x), _p(out), n, h, w, c, _stream()), ["avgpool2_fwd_kernel"], rid, [out])
    if tier == "exact":
        _equal(out.view, ref["p"], rid)
    else:
        err = np.abs(_host(out.view) - ref["p"]).max()
        print(rid, "abs err", err)
        assert err <= 1e-7, (rid, err)                            # test_gpu_ops.py::test_avgpool_guide_pyramid, uniform [0, 1)
    if rid in WRAP:
        assert torch.equal(ops.avgpool2_fwd(x.view), out.view)


@pytest.mark.parametrize("rid,storage,tier", _params("ig"))
def test_image_gradients_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    n, h, w, c = p["n"], p["h"], p["w"], p["c"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    x, out = r.i(a["x"]), r.o((n, h, w, 3 * c))
    r.go(lambda: lib().unetk_image_gradients(_p(x), _p(out), n, h, w, c, _stream()), ["image_gradients_kernel"], rid, [out])
    # one fp32 subtraction is correctly rounded: float64 rounded once (exact tier: nothing to round)
    _equal(out.view, ref["out"] if tier == "exact" else T.image_gradients(a["x"].astype(np.float32)).astype(np.float64), rid)
    if rid in WRAP:
        assert torch.equal(ops.image_gradients(x.view), out.view)


@pytest.mark.parametrize("rid,storage,tier", _params("sobel"))
def test_sobel_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    n, h, w, c, ch = p["n"], p["h"], p["w"], p["c"], p["ch"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    x, out = r.i(a["x"]), r.o((n, h, w, c + 2))
    r.go(lambda: lib().unetk_sobel_concat(_p(x), _p(out), n, h, w, c, ch, _stream()), ["sobel_concat_kernel"], rid, [out])
    if tier == "exact":
        _equal(out.view, ref["out"], rid)
    else:
        _equal(out.view[..., :c], ref["out"][..., :c], rid + " copy")
        _rel(out.view, ref["out"], rid, 1e-6)     # the whole tensor, as test_gpu_interunet.py::test_sobel_concat_kernel (2 x 2: zero edges)
    if rid in WRAP:
        assert torch.equal(ops.sobel_concat(x.view, ch), out.view)


@pytest.mark.parametrize("rid,storage,tier", _params("flip"))
def test_flip_axpy_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    n, h, w, c = p["n"], p["h"], p["w"], p["c"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    x = r.i(a["x"])
    out = r.o((n, h, w, c), init=a["out0"] if p["acc"] else None)
    r.go(lambda: lib().unetk_flip_axpy(_p(x), _p(out), n, h, w, c, p["fh"], p["fw"], p["scale"], p["acc"], _stream()),
         ["flip_axpy_kernel"], rid, [out])
    if tier == "exact" or not p["acc"]:
        _equal(out.view, ref["out"], rid)                       # scale is a power of two: the product is exact in both tiers
    else:
        # the product is exact, the sum rounds once -- or not at all when the compiler contracts it; either way within one fp32
        # ulp of the larger of |result| and the two terms
        mag = np.maximum(np.abs(ref["out"]), np.maximum(np.abs(ref["out"] - a["out0"]), np.abs(a["out0"])))
        assert (np.abs(_host(out.view) - ref["out"]) <= 2.0 ** -23 * mag).all(), rid
    if rid in WRAP:
        o2 = out.view.clone() if not p["acc"] else _dev(a["out0"])
        ops.flip_axpy(x.view, o2, p["fh"], p["fw"], p["scale"], bool(p["acc"]))
        assert torch.equal(o2, out.view)


@pytest.mark.parametrize("rid,storage,tier", _params("moments"))
def test_guide_moments_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    n, hw, g, ps = p["n"], p["hw"], p["g"], p["ps"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    guide, out = r.i(a["guide"]), r.o((n if ps else 1, g + g * g))
    r.go(lambda: lib().unetk_guide_moments(_p(guide), n, hw, g, ps, _p(out), _stream()), ["guide_moments_kernel"], rid, [out])
    if tier == "exact":
        _equal(out.view, T.f32(ref["out"]), rid)                # integer sums in float64, one division, one rounding to fp32
    else:
        # float64 accumulation in another order: 2^-50 of the mean of |g_i g_j| at the most; then the one rounding to fp32
        err = np.abs(_host(out.view) - ref["out"])
        assert (err <= 2.0 ** -24 * np.abs(ref["out"]) * (1 + 1e-6) + 1e-12 * max(1.0, np.abs(a["guide"]).max() ** 2)).all(), (rid, err.max())
    if rid in WRAP:
        assert torch.equal(ops.guide_moments(guide.view.reshape(n, hw, 1, g), bool(ps)).reshape(out.view.shape), out.view)


# ------------------------------------------------------------------ spatial mean
@pytest.mark.parametrize("rid,storage,tier", _params("smean"))
def test_spatial_mean_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    n, hw, c = p["n"], p["hw"], p["c"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    x, dy = r.i(a["x"]), r.i(a["dy"])
    y, dx = r.o((n, c)), r.o((n, hw, c))
    r.go(lambda: lib().unetk_spatial_mean_fwd(_p(x), _p(y), n, hw, c, _stream()), ["spatial_mean_fwd_kernel"], rid + " fwd", [y])
    if tier == "exact":
        _equal(y.view, T.f32(ref["y"]), rid + " y")             # an exact sum, one division
    else:
        _rel(y.view, ref["y"], rid + " y", T.SPATIAL_MEAN_REL)
    r.go(lambda: lib().unetk_spatial_mean_bwd(_p(dy), _p(dx), n, hw, c, _stream()), ["spatial_mean_bwd_kernel"], rid + " bwd", [dx])
    pow2 = hw & (hw - 1) == 0
    _equal(dx.view, ref["dx"] if (pow2 and tier == "exact") else T.spatial_mean_bwd_f32(a["dy"], hw), rid + " dx")
    if rid in WRAP:
        xt = x.view.clone().reshape(n, hw, 1, c).requires_grad_()
        yt = ops.SpatialMean.apply(xt)
        yt.backward(dy.view.clone())
        assert torch.equal(yt.detach(), y.view) and torch.equal(xt.grad.reshape(n, hw, c), dx.view)


# ------------------------------------------------------------------ FC
def _cmp(got, want, exact, what, bound=T.FC_REL):
    if exact:
        _equal(got, want, what)
    else:
        _rel(got, want, what, bound)


@pytest.mark.parametrize("rid,storage,tier", _params("fc"))
def test_fc_row(ops, rid, storage, tier):
    row = T.BY_ID[rid]
    p = row.p
    b, k, n, relu = p["b"], p["k"], p["n"], p["relu"]
    a, ref = _case(row, tier)
    ex = tier == "exact"
    r = Run(ops)
    x, w, dy = r.i(a["x"]), r.i(a["w"]), r.i(a["dy"])
    bias = r.i(a["b"]) if p["bias"] else None
    y = r.o((b, n))
    mask = r.o((b, n)) if p["keep"] is not None else None
    keep = p["keep"] if p["keep"] is not None else 1.0
    r.go(lambda: lib().unetk_fc_fwd(_p(x), _p(w), _p(bias), _p(y), _p(mask), b, k, n, relu, keep, T.SEED, _stream()),
         ["fc_fwd_kernel"], rid + " fwd", [y] + ([mask] if mask else []))
    if mask:
        _equal(mask.view, a["mask"], rid + " mask (element r * n + o of the counter RNG)")
    _cmp(y.view, ref["y"], ex, rid + " y")
    if ex and relu == 1:
        wrong = T.fc(a, 1, ge=True)
        assert (ref["pre"] == 0).any() and any(not np.array_equal(wrong[q], ref[q]) for q in ("db", "dw", "dx") if p.get(q, True))
    yin = r.i(_host(y.view))
    min_ = r.i(_host(mask.view)) if mask else None
    dx = r.o((b, k)) if p["dx"] else None
    dw = r.o((k, n))
    db = r.o((n,)) if p["db"] else None
    ws = r.ws(b * n * 4)                                         # include/unetk.h: dpre_ws = [B][n] floats
    outs = [o for o in (dx, dw, db) if o is not None]
    r.go(lambda: lib().unetk_fc_bwd(_p(x), _p(w), _p(yin), _p(min_), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), b, k, n, relu, _stream()),
         ["fc_bwd_pre_kernel", "fc_bwd_w_kernel"] + (["fc_bwd_x_kernel"] if dx else []), rid + " bwd", outs)
    _cmp(dw.view, ref["dw"], ex, rid + " dw")
    if dx:
        _cmp(dx.view, ref["dx"], ex, rid + " dx")
    if db:
        _cmp(db.view, ref["db"], ex, rid + " db")
    if rid in WRAP:
        xt, wt, bt = (t.view.clone().requires_grad_() for t in (x, w, bias))
        yt = ops.FullyConnected.apply(xt, wt, bt, relu, p["keep"], T.SEED)
        yt.backward(dy.view.clone())
        assert torch.equal(yt.detach(), y.view) and torch.equal(xt.grad, dx.view) and torch.equal(wt.grad, dw.view)
        assert torch.equal(bt.grad, db.view)


# ------------------------------------------------------------------ conv1d and the 1-D max-pool
@pytest.mark.parametrize("rid,storage,tier", _params("conv1d"))
def test_conv1d_row(ops, rid, storage, tier):
    row = T.BY_ID[rid]
    p = row.p
    b, l, ci, co, k, relu = p["b"], p["l"], p["ci"], p["co"], p["k"], p["relu"]
    a, ref = _case(row, tier)
    ex = tier == "exact"
    r = Run(ops)
    x, w, dy = r.i(a["x"]), r.i(a["w"]), r.i(a["dy"])
    bias = r.i(a["b"]) if p["bias"] else None
    y = r.o((b, l, co))
    r.go(lambda: lib().unetk_conv1d_fwd(_p(x), _p(w), _p(bias), _p(y), b, l, ci, co, k, relu, _stream()), ["conv1d_fwd_kernel"],
         rid + " fwd", [y])
    _cmp(y.view, ref["y"], ex, rid + " y")
    if ex and relu == 1:
        wrong = T.conv1d(a, k, 1, ge=True)
        assert (ref["pre"] == 0).any() and any(not np.array_equal(wrong[q], ref[q]) for q in ("db", "dw", "dx") if p.get(q, True))
    yin = r.i(_host(y.view))
    dx = r.o((b, l, ci)) if p["dx"] else None
    dw = r.o((k, ci, co))
    db = r.o((co,)) if p["db"] else None
    ws = r.ws(b * l * co * 4)                                    # include/unetk.h: dpre_ws = [B][L][Cout] floats
    outs = [o for o in (dx, dw, db) if o is not None]
    r.go(lambda: lib().unetk_conv1d_bwd(_p(x), _p(w), _p(yin), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), b, l, ci, co, k, relu, _stream()),
         ["conv1d_bwd_pre_kernel", "conv1d_bwd_w_kernel"] + (["conv1d_bwd_x_kernel"] if dx else []), rid + " bwd", outs)
    _cmp(dw.view, ref["dw"], ex, rid + " dw")
    if dx:
        _cmp(dx.view, ref["dx"], ex, rid + " dx")
    if db:
        _cmp(db.view, ref["db"], ex, rid + " db")
    if rid in WRAP:
        xt, wt, bt = (t.view.clone().requires_grad_() for t in (x, w, bias))
        yt = ops.Conv1d.apply(xt, wt, bt, bool(relu))
        yt.backward(dy.view.clone())
        assert torch.equal(yt.detach(), y.view) and torch.equal(xt.grad, dx.view) and torch.equal(wt.grad, dw.view)
        assert torch.equal(bt.grad, db.view)


@pytest.mark.parametrize("rid,storage,tier", _params("mp1"))
def test_maxpool1d_row(ops, rid, storage, tier):
    p = T.BY_ID[rid].p
    b, l, c = p["b"], p["l"], p["c"]
    a, ref = _case(T.BY_ID[rid], tier)
    r = Run(ops)
    x, dy = r.i(a["x"]), r.i(a["dy"])
    y, dx = r.o((b, (l + 1) // 2, c)), r.o((b, l, c))
    r.go(lambda: lib().unetk_maxpool1d_fwd(_p(x), _p(y), b, l, c, _stream()), ["maxpool1d_fwd_kernel"], rid + " fwd", [y])
    _equal(y.view, ref["y"], rid + " y")
    r.go(lambda: lib().unetk_maxpool1d_bwd(_p(x), _p(dy), _p(dx), b, l, c, _stream()), ["maxpool1d_bwd_kernel"], rid + " bwd", [dx])
    _equal(dx.view, ref["dx"], rid + " dx")
    if rid in WRAP:
        xt = x.view.clone().requires_grad_()
        yt = ops.MaxPool1d.apply(xt)
        yt.backward(dy.view.clone())
        assert torch.equal(yt.detach(), y.view) and torch.equal(xt.grad, dx.view)


# ------------------------------------------------------------------ boundary weights
@pytest.mark.parametrize("rid", [r.id for r in T.rows("boundary")])
def test_boundary_weights_row(ops, rid):
    row = T.BY_ID[rid]
    n, h, w = row.p["n"], row.p["h"], row.p["w"]
    lab = T.boundary_labels(row)
    r = Run(ops)
    labels, wmap = r.labels(lab), r.o((n, h, w))
    nbytes = int(lib().unetk_boundary_weights_ws_bytes(n, h, w))
    assert nbytes == T.boundary_ws_bytes(n, h, w)
    ws = r.ws(nbytes)
    r.go(lambda: lib().unetk_boundary_weights(_p(labels), n, h, w, _p(wmap), _p(ws), nbytes, _stream()),
         ["edt_columns_kernel", "edt_rows_kernel", "edt_normalise_kernel"], rid, [wmap])
    got = _host(wmap.view)
    np.testing.assert_allclose(got, T.boundary_weights(lab), rtol=T.BOUNDARY_RTOL, err_msg=rid)
    np.testing.assert_allclose(got.mean(axis=(1, 2)), 1.0, rtol=T.BOUNDARY_RTOL)
    if row.p["kind"] == "ringfree":                              # ratios between pixels: the image's scale cancels
        v = T.boundary_ringfree_unscaled(h, w)
        for i in range(n):
            np.testing.assert_allclose(got[i] / got[i, 0, 0], v / v[0, 0], rtol=T.BOUNDARY_RTOL)
    if rid in WRAP:
        assert torch.equal(ops.boundary_weights(torch.from_numpy(lab).cuda()), wmap.view)


# ------------------------------------------------------------------ refusals: the code, an empty trace, untouched outputs
# entry point -> argument list: (name, "in" | "out" | "in?" | "out?" (nullable) | "ws" | "v", shape / bytes / value)
_POOL_F = [("x", "in", (2, 4, 4, 8)), ("x_stride", "v", 8), ("p", "out", (2, 2, 2, 8)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("C", "v", 8)]
_POOL_B = [("x", "in", (2, 4, 4, 8)), ("x_stride", "v", 8), ("p", "in", (2, 2, 2, 8)), ("dp", "in", (2, 2, 2, 8)), ("add", "in?", (2, 4, 4, 8)),
           ("add_stride", "v", 8), ("dx", "out", (2, 4, 4, 8)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("C", "v", 8)]
_IMG = [("x", "in", (2, 4, 4, 2)), ("out", "out", (2, 4, 4, 6)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("C", "v", 2)]
_FC_DIMS = [("B", "v", 2), ("k", "v", 3), ("n", "v", 4)]
_C1_DIMS = [("B", "v", 2), ("L", "v", 3), ("Cin", "v", 2), ("Cout", "v", 4)]
ENTRY = {
    "unetk_maxpool2_fwd": (F32, _POOL_F), "unetk_maxpool2_fwd_bf16": (BF16, _POOL_F),
    "unetk_maxpool2_bwd": (F32, _POOL_B), "unetk_maxpool2_bwd_bf16": (BF16, _POOL_B),
    "unetk_avgpool2_fwd": (F32, [("x", "in", (2, 4, 4, 2)), ("p", "out", (2, 2, 2, 2)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("C", "v", 2)]),
    "unetk_image_gradients": (F32, _IMG),
    "unetk_sobel_concat": (F32, [("x", "in", (2, 4, 4, 2)), ("out", "out", (2, 4, 4, 4)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("C", "v", 2),
                                 ("ch", "v", 1)]),
    "unetk_flip_axpy": (F32, [("x", "in", (2, 4, 4, 2)), ("out", "out", (2, 4, 4, 2)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("C", "v", 2),
                              ("flip_h", "v", 1), ("flip_w", "v", 0), ("scale", "v", 1.0), ("accumulate", "v", 0)]),
    "unetk_guide_moments": (F32, [("guide", "in", (2, 16, 5)), ("N", "v", 2), ("HW", "v", 16), ("G", "v", 2), ("per_sample", "v", 1),
                                  ("out", "out", (2, 30))]),
    "unetk_spatial_mean_fwd": (F32, [("x", "in", (2, 4, 8)), ("y", "out", (2, 8)), ("N", "v", 2), ("HW", "v", 4), ("C", "v", 8)]),
    "unetk_spatial_mean_bwd": (F32, [("dy", "in", (2, 8)), ("dx", "out", (2, 4, 8)), ("N", "v", 2), ("HW", "v", 4), ("C", "v", 8)]),
    "unetk_fc_fwd": (F32, [("x", "in", (2, 3)), ("w", "in", (3, 4)), ("b", "in?", (4,)), ("y", "out", (2, 4)), ("mask", "out?", (2, 4))] + _FC_DIMS
                     + [("relu", "v", 1), ("keep_prob", "v", 0.5), ("seed", "v", 7)]),
    "unetk_fc_bwd": (F32, [("x", "in", (2, 3)), ("w", "in", (3, 4)), ("y", "in", (2, 4)), ("mask", "in?", (2, 4)), ("dy", "in", (2, 4)),
                           ("dx", "out?", (2, 3)), ("dw", "out", (3, 4)), ("db", "out?", (4,)), ("dpre_ws", "ws", 32)] + _FC_DIMS + [("relu", "v", 1)]),
    "unetk_conv1d_fwd": (F32, [("x", "in", (2, 3, 2)), ("w", "in", (3, 2, 4)), ("b", "in?", (4,)), ("y", "out", (2, 3, 4))] + _C1_DIMS
                         + [("k", "v", 3), ("relu", "v", 1)]),
    "unetk_conv1d_bwd": (F32, [("x", "in", (2, 3, 2)), ("w", "in", (3, 2, 4)), ("y", "in", (2, 3, 4)), ("dy", "in", (2, 3, 4)), ("dx", "out?", (2, 3, 2)),
                               ("dw", "out", (3, 2, 4)), ("db", "out?", (4,)), ("dpre_ws", "ws", 96)] + _C1_DIMS + [("k", "v", 3), ("relu", "v", 1)]),
    "unetk_maxpool1d_fwd": (F32, [("x", "in", (2, 4, 2)), ("y", "out", (2, 2, 2)), ("B", "v", 2), ("L", "v", 4), ("C", "v", 2)]),
    "unetk_maxpool1d_bwd": (F32, [("x", "in", (2, 4, 2)), ("dy", "in", (2, 2, 2)), ("dx", "out", (2, 4, 2)), ("B", "v", 2), ("L", "v", 4), ("C", "v", 2)]),
    "unetk_boundary_weights": (F32, [("labels", "in", (2, 4, 4)), ("N", "v", 2), ("H", "v", 4), ("W", "v", 4), ("wmap", "out", (2, 4, 4)),
                                     ("ws", "ws", T.boundary_ws_bytes(2, 4, 4)), ("ws_bytes", "v", T.boundary_ws_bytes(2, 4, 4))]),
}
_POOLS = ("unetk_maxpool2_fwd", "unetk_maxpool2_fwd_bf16", "unetk_maxpool2_bwd", "unetk_maxpool2_bwd_bf16")
_POOLS_B = _POOLS[2:]
REFUSALS = (
    [(e, "c_mod4", dict(C=6), E_UNSUPPORTED) for e in _POOLS] + [(e, "x_stride_mod4", dict(x_stride=10), E_UNSUPPORTED) for e in _POOLS]
    + [(e, "x_stride_below_c", dict(x_stride=4), E_BADARG) for e in _POOLS] + [(e, "h_below_2", dict(H=1), E_BADARG) for e in _POOLS]
    + [(e, "w_below_2", dict(W=1), E_BADARG) for e in _POOLS] + [(e, "x_off_by_one_element", dict(x="+1"), E_BADARG) for e in _POOLS]
    + [(e, "p_off_by_one_element", dict(p="+1"), E_BADARG) for e in _POOLS]
    + [(e, "odd_h", dict(H=3), E_UNSUPPORTED) for e in _POOLS_B] + [(e, "odd_w", dict(W=3), E_UNSUPPORTED) for e in _POOLS_B]
    + [(e, "add_stride_below_c", dict(add_stride=4), E_BADARG) for e in _POOLS_B] + [(e, "add_stride_mod4", dict(add_stride=10), E_BADARG) for e in _POOLS_B]
    + [(e, "add_off_by_one_element", dict(add="+1"), E_BADARG) for e in _POOLS_B] + [(e, "dx_off_by_one_element", dict(dx="+1"), E_BADARG) for e in _POOLS_B]
    + [("unetk_avgpool2_fwd", "odd_h", dict(H=3), E_UNSUPPORTED), ("unetk_avgpool2_fwd", "odd_w", dict(W=3), E_UNSUPPORTED),
       ("unetk_sobel_concat", "h_below_2", dict(H=1), E_BADARG), ("unetk_sobel_concat", "w_below_2", dict(W=1), E_BADARG),
       ("unetk_sobel_concat", "ch_negative", dict(ch=-1), E_BADARG), ("unetk_sobel_concat", "ch_is_c", dict(ch=2), E_BADARG),
       ("unetk_flip_axpy", "x_is_out", dict(out="=x"), E_BADARG),
       ("unetk_guide_moments", "g_5", dict(G=5), E_BADARG), ("unetk_guide_moments", "g_0", dict(G=0), E_BADARG),
       ("unetk_spatial_mean_fwd", "n_65536", dict(N=65536), E_BADARG),
       ("unetk_fc_fwd", "keep_0_with_mask", dict(keep_prob=0.0), E_BADARG), ("unetk_fc_fwd", "keep_above_1_with_mask", dict(keep_prob=1.5), E_BADARG),
       ("unetk_fc_fwd", "b_65536", dict(B=65536), E_BADARG), ("unetk_fc_bwd", "b_65536", dict(B=65536), E_BADARG),
       ("unetk_fc_bwd", "k_65536", dict(k=65536), E_BADARG),
       ("unetk_fc_fwd", "sigmoid_with_mask", dict(relu=2), E_UNSUPPORTED), ("unetk_fc_bwd", "sigmoid_with_mask", dict(relu=2), E_UNSUPPORTED),
       ("unetk_conv1d_fwd", "k_2", dict(k=2), E_UNSUPPORTED), ("unetk_conv1d_fwd", "k_5", dict(k=5), E_UNSUPPORTED),
       ("unetk_conv1d_bwd", "k_2", dict(k=2), E_UNSUPPORTED), ("unetk_conv1d_bwd", "k_5", dict(k=5), E_UNSUPPORTED),
       ("unetk_boundary_weights", "w_12289", dict(W=12289, ws_bytes=1 << 30), E_UNSUPPORTED),
       ("unetk_boundary_weights", "ws_16_bytes_short", dict(ws_bytes=T.boundary_ws_bytes(2, 4, 4) - 16), E_WORKSPACE)]
    + [(e, "null_" + name, {name: None}, E_BADARG) for e, (_, args) in sorted(ENTRY.items()) for name, kind, _ in args if kind in ("in", "out", "ws")])


@pytest.mark.parametrize("entry,name,over,code", REFUSALS, ids=["%s-%s" % (r[0][6:], r[1]) for r in REFUSALS])
def test_refusal(ops, entry, name, over, code):
    """Buffers of the ordinary (valid) size: a refused descriptor, however large, must not reach a kernel."""
    dtype, spec = ENTRY[entry]
    esize = 2 if dtype == BF16 else 4
    bufs, outs, wss, argv = {}, [], [], []
    for arg, kind, val in spec:
        if kind == "v":
            continue
        if kind == "ws":
            bufs[arg] = guardbuf.GuardedWorkspace(val)
            wss.append(bufs[arg])
        elif kind.startswith("in"):
            bufs[arg] = guardbuf.guarded_input(torch.ones(val, device="cuda").to(dtype if arg != "labels" else F32))
        else:
            bufs[arg] = guardbuf.guarded(val, dtype)
            outs.append(bufs[arg])
    for arg, kind, val in spec:
        if kind == "v":
            argv.append(over.get(arg, val))
            continue
        o = over.get(arg, "")
        if arg in over and o is None:
            argv.append(None)
        elif o == "+1":
            argv.append(ctypes.c_void_p(bufs[arg].ptr() + esize))
        elif isinstance(o, str) and o.startswith("="):
            argv.append(_p(bufs[o[1:]]))
        else:
            argv.append(_p(bufs[arg]))
    rc, names = _trace(ops, lambda: getattr(lib(), entry)(*(argv + [_stream()])))
    assert rc == code and names == [], (entry, name, rc, names)
    for o in outs:
        assert o.changed_anywhere() == 0, (entry, name)
    for w in wss:
        assert w.guard_intact() and torch.equal(w.buf, w.snap), (entry, name)


def test_fc_sigmoid_with_a_mask_is_refused_by_the_wrapper(ops):
    """The backward would multiply by y (1 - y) of the MASKED y = sigmoid(acc) m where m s (1 - s) belongs (keep 1/2: 2s (1 - 2s) for
    s (1 - s)); no model drops out a gate, so both entry points return UNETK_E_UNSUPPORTED before any launch (include/unetk.h: the two
    sigmoid_with_mask rows of test_refusal) and ops.FullyConnected raises."""
    from boxsegliver_amd import _abi
    x, w, b = torch.ones(2, 3, device="cuda"), torch.ones(3, 4, device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(_abi.UnetkError):
        ops.FullyConnected.apply(x, w, b, 2, 0.5, 7)
