"""The norm apply / backward kernels of csrc/norm.hip on every dispatch path, through the C ABI (table: tests/norm_paths.py).

Every row asserts the launch trace in order (reducer launches included), runs in guarded buffers (tests/guardbuf.py) with a
workspace of exactly unetk_norm_bwd_ws_bytes(d) bytes that starts as NaN patterns, and runs every backward twice, bit-equal.

Exact tier.  scale / shift / mean / rstd are INPUTS of the entry points, so the test supplies them: y integers in [-4, 4], mean
integers in [-2, 2], rstd and den in {1/2, 1, 2}, gamma in {+-1/2, +-1, 2} (channel 3: 0), beta / gw / gb / post shift eighths,
guide integers in [0, 3], post slopes in {0, 1}, alpha 1/4, dz / dp / dskip integers in [-2, 2], keep in {1/2, 1/4}.  Then
  * z (and the pooled tensor) equal float64 bit for bit -- under bf16 storage float64 rounded once to bf16;
  * every SUM output (dbeta, dgamma, dgw, dgb, dden, the per-sample dgw / dgb, the post block's rows) is a sum of exact products
    below 2^24 units and equals float64 bit for bit in any order;
  * dy multiplies by 1 / Ps: it is compared bit for bit on the rows marked xdy (Ps a power of two, every intermediate
    representable) and at the bound tier's bound everywhere else.  A normaliser is not a convolution of small integers:
    1 / Ps, like 1 / sqrt(var + eps), is a rounded value unless chosen not to be.
tests/test_norm_paths_host.py asserts representability and the 2^24 bound on the float64 side, so a badly chosen row fails as a row.
The fixed 0.2 slope of guide_leaky == 1 is no binary fraction: those rows compare at the bounds in both tiers.

Bound tier (same rows, Gaussian inputs of test_gpu_ops.py::test_norm_relu_forward_backward, the float64 restatement
oracle/norm_unit.py): z 1e-5, dy and parameter gradients 2e-5 (test_gpu_ops.py); bf16 storage: stored values
within one bf16 ulp and all but 5e-3 of them the exact rounding (test_gpu_bf16s.py).  Every row runs in both tiers, the grid-cap
rows included (C = 516 there: a row group of 516 elements instead of 1024).  No row carries more than 1.7 x 10^4 terms per
channel, and a thread's own fp32 chain is a few terms long (the rest is summed over the block in LDS and over the grid in
float64): none needs the long-chain bound, and each passes the plain one.
"""
import ctypes

import numpy as np
import pytest
import torch

import guardbuf
import norm_paths as T
from oracle import norm_unit

pytestmark = pytest.mark.gpu

E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
ULP = 2.0 ** -8


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


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dtype)


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def _sd(storage):
    return torch.bfloat16 if storage == T.BF16S else torch.float32


def _stored_ok(got, ref64, what, flips=5e-3):
    """test_gpu_bf16s.py::_stored_ok: every element within one bf16 ulp, all but `flips` of them the exact rounding.
    flips=None (the exact tier's dy on rows that are not xdy): with the exact tier's inputs the true dy is a ratio of small integers
    and may sit ON a bf16 rounding boundary, where the fp32 rounding of k / Ps decides the direction.  So instead of a share, every
    element whose float64 value is farther than tol = 2^-20 max |dy| from a boundary must be the exact rounding.  tol from the
    kernel's expression sc0 (dt - k1 / Ps - xhat (k2 / Ps)): dt, xhat, k1, k2 and sc0 (a power of two or zero) are exact, so the
    error is five fp32 roundings of intermediates of the size of max |dy| (|sc0| <= 4 takes the bracket to dy): tol = 16 x 2^-24
    max |dy| leaves a factor of three over 5 x 2^-24."""
    got = np.asarray(got, np.float64)
    big = np.abs(ref64) > 1e-3 * np.abs(ref64).max()
    if big.any():
        err = np.abs(got - ref64)[big] / np.abs(ref64)[big]
        print(what, "bf16 rel err", err.max())
        assert err.max() <= 1.01 * ULP, (what, err.max())
    exact = got == T.round_bf16(ref64)
    print(what, "exactly rounded share", exact.mean())
    if flips is None:
        tol = 2.0 ** -20 * np.abs(ref64).max()
        decided = T.round_bf16(ref64 - tol) == T.round_bf16(ref64 + tol)
        print(what, "share within tol of a rounding boundary", 1.0 - decided.mean())
        assert exact[decided].all(), (what, int((~exact[decided]).sum()))
    else:
        assert exact.mean() > 1.0 - flips, (what, exact.mean())


def _cmp_tensor(got_t, ref64, storage, bitwise, bound, what, flips=5e-3):
    """A stored activation-like tensor (z, dy, pooled) against float64."""
    got = got_t.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    if bitwise:
        want = T.round_bf16(ref64) if storage == T.BF16S else ref64
        bad = int((got != want).sum())
        assert bad == 0, "{}: {} of {} elements differ from float64, first at {}".format(
            what, bad, got.size, np.argwhere(got != want)[:3].tolist())
    elif storage == T.BF16S:
        _stored_ok(got, ref64, what, flips)
    else:
        e = _rel(got, ref64)
        print(what, "rel err", e)
        assert e < bound, (what, e)


def _cmp_sum(got_t, ref64, bitwise, what, bound=2e-5):
    got = got_t.cpu().numpy().astype(np.float64).reshape(np.shape(ref64))
    if bitwise:
        assert np.array_equal(got, ref64), "{}: {} sums differ from float64".format(what, int((got != ref64).sum()))
    else:
        e = _rel(got, ref64)
        print(what, "rel err", e)
        assert e < bound, (what, e)


def make_desc(row, st, **over):
    from boxsegliver_amd import _abi
    f = dict(N=row.n, HW=row.hw, C=row.c, per_sample=row.ps, z_stride=row.c + row.zpad, guide_ch=row.g,
             gw_stride=row.gstride if (row.g or row.gbare) else 0, gw_coff=row.coff, affine_only=int(row.affine),
             guide_leaky=row.leaky, storage=st, guide_alpha=0.0, dropout_keep=row.keep, dropout_seed=T.SEED,
             guide_per_sample=int(row.gps))
    f.update(over)
    return _abi.NormDesc(f["N"], f["HW"], f["C"], f["per_sample"], f["z_stride"], f["guide_ch"], f["gw_stride"], f["gw_coff"],
                         f["affine_only"], f["guide_leaky"], f["storage"], f["guide_alpha"], f["dropout_keep"], f["dropout_seed"],
                         f["guide_per_sample"])


def _columns(a, row, lead):
    """[..., C] parameter rows -> [..., gw_stride] with the data at columns gw_coff .. and poison around them."""
    full = np.full(tuple(lead) + (row.gstride,), guardbuf.POISON, np.float32)
    full[..., row.coff:row.coff + row.c] = a
    return torch.from_numpy(full).cuda()


class Call(object):
    """The device side of one row: guarded buffers and the C calls."""

    def __init__(self, row, storage, a):
        self.row, self.storage, self.a = row, storage, a
        sd = _sd(storage)
        n, hw, c = row.n, row.hw, row.c
        self.d = make_desc(row, storage, guide_alpha=a["alpha"])
        self.y = guardbuf.guarded_input(_dev(a["y"], sd))
        self.dz = guardbuf.guarded_input(_dev(a["dz"], sd), pixel_stride=c + row.dzpad, coff=row.dzpad // 2 // 4 * 4)
        self.stat = [guardbuf.guarded_input(_dev(a[k])) for k in ("scale", "shift", "mean", "rstd")]
        self.den = guardbuf.guarded_input(_dev(a["den"])) if a["den"] is not None else None
        self.guide = guardbuf.guarded_input(_dev(a["guide"])) if row.g else None
        ng = n if row.gps else 1
        self.gw = _columns(a["gw"], row, (ng, row.g)) if row.g else None
        self.gb = None
        if a["gb"] is not None:
            self.gb = _columns(a["gb"], row, (ng, 4) if row.leaky == 3 else (ng,))
        self.z = guardbuf.guarded((n, hw, c), sd, pixel_stride=c + row.zpad, coff=row.zpad // 2 // 4 * 4)
        self.dy = guardbuf.guarded((n, hw, c), sd)
        self.dgamma, self.dbeta = guardbuf.guarded((c,)), guardbuf.guarded((c,))
        self.dden = guardbuf.guarded((n, c)) if row.den else None
        self.dgw = guardbuf.guarded((ng, row.g, c)) if row.g else None
        self.dgb = guardbuf.guarded(((ng, 4, c) if row.leaky == 3 else (ng, c))) if a["gb"] is not None else None
        self.outs = [o for o in (self.dy, self.dgamma, self.dbeta, self.dden, self.dgw, self.dgb) if o is not None]
        self.ins = [self.y, self.dz] + self.stat + [i for i in (self.den, self.guide) if i is not None]
        L = lib()
        self.ws_bytes = int(L.unetk_norm_bwd_ws_bytes(ctypes.byref(self.d)))
        self.ws = guardbuf.GuardedWorkspace(self.ws_bytes)
        self.pre = None
        if row.kind == "pool":
            self.dp = guardbuf.guarded_input(_dev(a["dp"], sd))
            self.pooled = guardbuf.guarded((n, hw // 4, c), sd)
            self.ins.append(self.dp)

    def set_pre(self, part):
        flat = torch.full((part.size + 8,), guardbuf.POISON, device="cuda")
        off = 4 if self.row.prealign else 1                      # 16-byte aligned, or 4-byte aligned only
        flat[off:off + part.size] = _dev(part.reshape(-1))
        self.pre = flat[off:]
        assert (self.pre.data_ptr() % 16 == 0) == self.row.prealign

    def apply(self):
        s = self.stat
        if self.row.kind == "pool":
            return lib().unetk_norm_apply_relu_pool(ctypes.byref(self.d), self.row.w, _p(self.y), _p(s[0]), _p(s[1]), _p(self.z),
                                                    _p(self.pooled), _stream())
        return lib().unetk_norm_apply_relu(ctypes.byref(self.d), _p(self.y), _p(s[0]), _p(s[1]), _p(self.den), _p(self.guide),
                                           _p(self.gw), _p(self.gb), _p(self.z), _stream())

    def bwd(self, ws_bytes=None, d=None, dz_stride=None):
        s, r = self.stat, self.row
        for o in self.outs:
            o.reset()
        self.ws.fill(0xFF)                                       # NaN patterns: nothing may be read before it is written
        d = self.d if d is None else d
        wsb = self.ws_bytes if ws_bytes is None else ws_bytes
        dzs = (r.c + r.dzpad) if dz_stride is None else dz_stride
        if r.kind == "pool":
            return lib().unetk_norm_relu_bwd_pool(ctypes.byref(d), r.w, _p(self.y), _p(self.dz), dzs, _p(self.dp), _p(s[0]),
                                                  _p(s[1]), _p(s[2]), _p(s[3]), _p(self.dy), _p(self.dgamma), _p(self.dbeta),
                                                  _p(self.ws), wsb, _stream())
        return lib().unetk_norm_relu_bwd_pre(ctypes.byref(d), _p(self.y), _p(self.dz), dzs, _p(s[0]), _p(s[1]), _p(s[2]), _p(s[3]),
                                             _p(self.den), _p(self.guide), _p(self.gw), _p(self.gb), _p(self.dy), _p(self.dgamma),
                                             _p(self.dbeta), _p(self.dden), _p(self.dgw), _p(self.dgb), _p(self.pre),
                                             r.pre if self.pre is not None else 0, _p(self.ws), wsb, _stream())

    def snapshot(self):
        return [o.flat.clone() for o in self.outs]

    def check_guards(self, what, outs=None):
        for o in (self.outs if outs is None else outs):
            assert o.check_untouched(), what + ": wrote outside an output view"
            assert o.unwritten() == 0, what + ": left output elements unwritten"
        for i in self.ins:
            assert i.changed_anywhere() == 0, what + ": changed an input"
        assert self.ws.guard_intact(), what + ": wrote outside the workspace"


def _cases(kind):
    out = []
    for r in T.ROWS:
        if r.kind != kind:
            continue
        for st in (T.FP32S, T.BF16S) if r.bf else (T.FP32S,):
            for tier in ("exact", "gauss"):
                out.append(pytest.param(r.id, st, tier, id="%s-%s-%s" % (r.id, "bf16s" if st else "fp32", tier)))
    return out


def _check_backward(c, ref, bitwise, what, tier):
    r, st = c.row, c.storage
    _cmp_tensor(c.dy.view, ref["dy"], st, bitwise and r.xdy, 2e-5, what + " dy", flips=None if tier == "exact" else 5e-3)
    _cmp_sum(c.dbeta.view, ref["dbeta"], bitwise, what + " dbeta")
    _cmp_sum(c.dgamma.view, ref["dgamma"], bitwise, what + " dgamma")
    if r.den:
        _cmp_sum(c.dden.view, ref["dden"], bitwise, what + " dden")
    if r.g:
        _cmp_sum(c.dgw.view, ref["dgw"], bitwise, what + " dgw")
    if c.dgb is not None:
        _cmp_sum(c.dgb.view, ref["dgb"], bitwise, what + " dgb")


@pytest.mark.parametrize("rid,storage,tier", _cases("unit"))
def test_unit_row(ops, rid, storage, tier):
    r = T.BY_ID[rid]
    a = T.make_inputs(r, tier, storage)
    ref = T.unit_reference(r, a)
    bitwise = tier == "exact" and T.exact_tier_is_bitwise(r)
    c = Call(r, storage, a)
    assert c.ws_bytes == T.ws_bytes(r)
    rc, names = _trace(ops, c.apply)
    assert rc == 0, rc
    _assert_trace(names, T.expected_apply(r, storage), rid + " apply")
    c.check_guards(rid + " apply", [c.z])
    _cmp_tensor(c.z.view, ref["z"], storage, bitwise, 1e-5, rid + " z")
    if r.pre:
        c.set_pre(T.pre_partials(r, ref))
    rc, names = _trace(ops, c.bwd)
    assert rc == 0, rc
    _assert_trace(names, T.expected_bwd(r, storage), rid + " backward")
    torch.cuda.synchronize()
    c.check_guards(rid + " backward")
    _check_backward(c, ref, bitwise, rid, tier)
    first = c.snapshot()
    assert c.bwd() == 0
    torch.cuda.synchronize()
    for o, f in zip(c.outs, first):
        assert torch.equal(o.bits(), o.bits(f)), rid + ": the backward is not bit-reproducible"


@pytest.mark.parametrize("rid,storage,tier", _cases("pool"))
def test_pool_row(ops, rid, storage, tier):
    r = T.BY_ID[rid]
    a = T.make_inputs(r, tier, storage)
    c = Call(r, storage, a)
    n, h, w = r.n, r.hw // r.w, r.w
    rc, names = _trace(ops, c.apply)
    assert rc == 0, rc
    _assert_trace(names, T.expected_apply(r, storage), rid + " apply+pool")
    c.check_guards(rid + " apply+pool", [c.z, c.pooled])
    bitwise = tier == "exact"
    if bitwise:
        ref = T.pool_reference(r, a, storage)
    else:
        # the device's own stored z decides the window (near-ties must not decide the test, test_gpu_pool_fused.py)
        fwd = T.unit_reference(r, a)
        z_dev = c.z.view.float().cpu().numpy().astype(np.float64)
        rnd = T.round_bf16 if storage == T.BF16S else (lambda v: v.astype(np.float32).astype(np.float64))
        dz = norm_unit.pool_route(z_dev, a["dz"], a["dp"], n, h, w, rnd)
        ref = T.unit_reference(r, a, dz=dz)
        ref["z"], ref["pooled"] = fwd["z"], norm_unit.pooled(z_dev, n, h, w)
    _cmp_tensor(c.z.view, ref["z"], storage, bitwise, 1e-5, rid + " z")
    got_p = c.pooled.view.float().cpu().numpy().astype(np.float64)
    assert np.array_equal(got_p, norm_unit.pooled(c.z.view.float().cpu().numpy(), n, h, w)), rid + ": pooled != max of the stored z"
    if bitwise:
        _cmp_tensor(c.pooled.view, ref["pooled"], storage, True, 0.0, rid + " pooled")
    rc, names = _trace(ops, c.bwd)
    assert rc == 0, rc
    _assert_trace(names, T.expected_bwd(r, storage), rid + " backward")
    torch.cuda.synchronize()
    c.check_guards(rid + " backward")
    _check_backward(c, ref, bitwise, rid, tier)
    first = c.snapshot()
    assert c.bwd() == 0
    torch.cuda.synchronize()
    for o, f in zip(c.outs, first):
        assert torch.equal(o.bits(), o.bits(f)), rid + ": the backward is not bit-reproducible"
    # the separate passes: unetk_maxpool2_bwd (+ dskip) then unetk_norm_relu_bwd.  The routed gradient is the same bit for bit;
    # the two channel sums are accumulated in another order, which the exact tier does not see.
    zc = c.z.view.reshape(n, h, w, r.c)
    dz_sep = ops.maxpool2_bwd(zc, c.pooled.view.reshape(n, h // 2, w // 2, r.c), c.dp.view.reshape(n, h // 2, w // 2, r.c),
                              add=c.dz.view.reshape(n, h, w, r.c))
    aff = torch.stack([s.view for s in (c.stat[2], c.stat[3], c.stat[0], c.stat[1])]).contiguous()      # mean, rstd, scale, shift
    d2 = make_desc(r, storage)
    dy2, dgamma2, dbeta2, _, _ = ops.norm_relu_bwd(d2, c.y.view.reshape(n, h, w, r.c).contiguous(), dz_sep.contiguous(), aff, True, True)
    if bitwise:
        assert torch.equal(dy2.reshape(n, r.hw, r.c), c.dy.view) and torch.equal(dgamma2, c.dgamma.view) and torch.equal(dbeta2, c.dbeta.view)
    else:
        sep = lambda u, v: float((u.double() - v.double()).norm() / v.double().norm())
        assert sep(dgamma2, c.dgamma.view) < 2e-6 and sep(dbeta2, c.dbeta.view) < 2e-6
        assert sep(dy2.reshape(n, r.hw, r.c), c.dy.view) < (2e-6 if storage == T.FP32S else 2e-3)


@pytest.mark.parametrize("rid,storage,tier", _cases("se"))
def test_se_row(ops, rid, storage, tier):
    """unetk_norm_se_bwd_add, unetk_norm_drop_pool, unetk_norm_se_bwd_add_drop: one launch group per sample."""
    r = T.BY_ID[rid]
    a = T.make_inputs(r, tier, storage)
    sd, t, ps = _sd(storage), T.tname(storage), bool(r.ps)
    bitwise = tier == "exact"
    d = make_desc(r, storage)
    y = guardbuf.guarded_input(_dev(a["y"], sd))
    stat = {k: guardbuf.guarded_input(_dev(a[k])) for k in ("mean", "rstd", "scale", "A", "k1", "k2")}
    L = lib()
    # dy += scale (A - xhat k2)
    dy = guardbuf.guarded_input(_dev(a["dz"], sd))
    rc, names = _trace(ops, lambda: L.unetk_norm_se_bwd_add(ctypes.byref(d), _p(y), _p(dy), _p(stat["mean"]), _p(stat["rstd"]),
                                                          _p(stat["scale"]), _p(stat["A"]), _p(stat["k2"]), _stream()))
    assert rc == 0, rc
    _assert_trace(names, ["norm_se_bwd_add_kernel<%s>" % t], rid)
    assert dy.check_untouched()
    _cmp_tensor(dy.view, norm_unit.se_add(a["y"], a["dz"], a["mean"], a["rstd"], a["scale"], a["A"], a["k2"], ps), storage, bitwise,
                2e-5, rid + " se_add")
    # sums of m xhat and of m
    sums = guardbuf.guarded((2, r.n, r.c))
    rc, names = _trace(ops, lambda: L.unetk_norm_drop_pool(ctypes.byref(d), _p(y), _p(stat["mean"]), _p(stat["rstd"]), _p(sums), _stream()))
    assert rc == 0, rc
    _assert_trace(names, ["norm_drop_pool_kernel<%s>" % t], rid)
    assert sums.check_untouched() and sums.unwritten() == 0
    want, _ = norm_unit.drop_pool(a["y"], a["mean"], a["rstd"], a["mask"], ps)
    _cmp_sum(sums.view[1], want[1], True, rid + " sum m")               # the mask sum is a sum of 0 | 1 / keep in both tiers
    _cmp_sum(sums.view[0], want[0], bitwise, rid + " sum m xhat")
    # dy += scale (m E - k1 - xhat k2)
    dy2 = guardbuf.guarded_input(_dev(a["dz"], sd))
    rc, names = _trace(ops, lambda: L.unetk_norm_se_bwd_add_drop(ctypes.byref(d), _p(y), _p(dy2), _p(stat["mean"]), _p(stat["rstd"]),
                                                               _p(stat["scale"]), _p(stat["A"]), _p(stat["k1"]), _p(stat["k2"]),
                                                               _stream()))
    assert rc == 0, rc
    _assert_trace(names, ["norm_se_bwd_add_drop_kernel<%s>" % t], rid)
    assert dy2.check_untouched()
    _cmp_tensor(dy2.view, norm_unit.se_add_drop(a["y"], a["dz"], a["mean"], a["rstd"], a["scale"], a["A"], a["k1"], a["k2"],
                                                a["mask"], ps), storage, bitwise, 2e-5, rid + " se_add_drop")
    for i in [y] + list(stat.values()):
        assert i.changed_anywhere() == 0


# ------------------------------------------------------------------ refusals
BASE = T._r("refuse_base", 2, 16, 24, False, T.PLAIN, ["w"])
REFUSALS = [
    # name, row overrides, descriptor overrides, call overrides, codes (apply, backward; None = that call is not refused), ws query 0
    ("c_mod4", dict(), dict(C=22), dict(), (E_UNSUPPORTED, E_UNSUPPORTED), True),
    ("c_1028", dict(), dict(C=1028, z_stride=1028), dict(dz_stride=1028), (E_UNSUPPORTED, E_UNSUPPORTED), True),
    ("z_stride_mod4", dict(), dict(z_stride=26), dict(), (E_UNSUPPORTED, None), False),
    ("dz_stride_mod4", dict(), dict(), dict(dz_stride=26), (None, E_UNSUPPORTED), False),
    ("guide_ch_5", dict(g=1), dict(guide_ch=5), dict(), (E_BADARG, E_BADARG), True),
    ("leaky_without_guide", dict(), dict(guide_leaky=1), dict(), (E_UNSUPPORTED, E_UNSUPPORTED), True),
    ("post_without_den", dict(g=1, leaky=3), dict(), dict(), (E_UNSUPPORTED, E_UNSUPPORTED), False),
    ("post_without_gb", dict(g=1, den=True, leaky=3), dict(), dict(no_gb=True), (E_BADARG, E_BADARG), False),
    ("post_with_pre", dict(g=1, den=True, leaky=3), dict(), dict(pre=2), (None, E_UNSUPPORTED), False),
    ("pre_with_guide", dict(g=1), dict(), dict(pre=2), (None, E_UNSUPPORTED), False),
    ("pre_with_density", dict(den=True), dict(), dict(pre=2), (None, E_UNSUPPORTED), False),
    ("pre_with_dropout", dict(keep=0.5), dict(), dict(pre=2), (None, E_UNSUPPORTED), False),
    ("pre_with_affine_only", dict(affine=True), dict(), dict(pre=2), (None, E_UNSUPPORTED), False),
    ("pre_rows_mod_l", dict(ps=1), dict(), dict(pre=3), (None, E_BADARG), False),
    ("keep_negative", dict(), dict(dropout_keep=-0.5), dict(), (E_BADARG, E_BADARG), True),
    ("keep_above_one", dict(), dict(dropout_keep=1.5), dict(), (E_BADARG, E_BADARG), True),
    ("dropout_bias_no_density", dict(g=1, keep=0.5), dict(), dict(), (None, E_UNSUPPORTED), False),
    ("gps_one_launch_group", dict(g=1, gps=True), dict(), dict(), (E_UNSUPPORTED, E_UNSUPPORTED), False),
    ("ws_16_short", dict(), dict(), dict(ws_short=16), (None, E_WORKSPACE), False),
    ("storage_bf16_operands", dict(), dict(storage=1), dict(), (E_BADARG, E_BADARG), True),
    ("storage_3", dict(), dict(storage=3), dict(), (E_BADARG, E_BADARG), True),
]


@pytest.mark.parametrize("name,rowo,desco,callo,codes,ws0", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(ops, name, rowo, desco, callo, codes, ws0):
    """Return code, an empty trace, untouched guarded outputs; the workspace query is 0 where the descriptor alone decides."""
    r = BASE._replace(id=name, **rowo)
    if r.g or r.gbare:
        r = r._replace(gstride=r.c)
    a = T.make_inputs(r, "exact", T.FP32S)
    c = Call(r, T.FP32S, a)                       # buffers of the VALID shape; the refused descriptor must not reach a kernel
    d = make_desc(r, T.FP32S, guide_alpha=a["alpha"], **desco)
    q = int(lib().unetk_norm_bwd_ws_bytes(ctypes.byref(d)))
    assert (q == 0) == ws0, (name, q)
    if "pre" in callo:
        r2 = r._replace(pre=callo["pre"])
        c.row = r2
        c.set_pre(np.zeros((2, callo["pre"], r.c)))
    if callo.get("no_gb"):
        c.gb = None                                # the guide is there, its bias block is not
    good = c.d
    if codes[0] is not None:
        c.d = d
        rc, names = _trace(ops, c.apply)
        assert rc == codes[0] and names == [], (name, rc, names)
        assert c.z.changed_anywhere() == 0
    c.d = good
    if codes[1] is not None:
        wsb = c.ws_bytes - callo.get("ws_short", 0)
        rc, names = _trace(ops, lambda: c.bwd(ws_bytes=wsb, d=d, dz_stride=callo.get("dz_stride")))
        assert rc == codes[1] and names == [], (name, rc, names)
        for o in c.outs:
            assert o.changed_anywhere() == 0, name
        assert c.ws.guard_intact()


POOL_BASE = T._r("refuse_pool", 2, 16, 24, False, "", ["w"], w=4, kind="pool")


@pytest.mark.parametrize("name,w,hw,desco", [("odd_w", 3, 12, {}), ("odd_h", 4, 12, {}), ("hw_mod_w", 6, 16, {}), ("w_below_2", 0, 16, {}),
                                             ("guide", 4, 16, dict(guide_ch=1)), ("dropout", 4, 16, dict(dropout_keep=0.5)),
                                             ("leaky", 4, 16, dict(guide_leaky=1)), ("c_mod4", 4, 16, dict(C=22))])
def test_pool_refusal(ops, name, w, hw, desco):
    a = T.make_inputs(POOL_BASE, "exact", T.FP32S)
    c = Call(POOL_BASE, T.FP32S, a)
    c.d = make_desc(POOL_BASE, T.FP32S, HW=hw, **desco)
    c.row = POOL_BASE._replace(w=w)
    rc, names = _trace(ops, c.apply)
    assert rc == E_UNSUPPORTED and names == [], (name, rc, names)
    assert c.z.changed_anywhere() == 0 and c.pooled.changed_anywhere() == 0
    rc, names = _trace(ops, lambda: c.bwd(d=c.d))
    assert rc == E_UNSUPPORTED and names == [], (name, rc, names)
    for o in c.outs:
        assert o.changed_anywhere() == 0, name


def test_side_pass_refusals(ops):
    r = T.BY_ID["se_n5_p3_c24"]
    a = T.make_inputs(r, "exact", T.FP32S)
    y, dy = _dev(a["y"]), guardbuf.guarded_input(_dev(a["dz"]))
    st = {k: _dev(a[k]) for k in ("mean", "rstd", "scale", "A", "k1", "k2")}
    sums = guardbuf.guarded((2, r.n, r.c))
    L = lib()
    for over, code in ((dict(C=22), E_UNSUPPORTED), (dict(dropout_keep=0.0), E_BADARG), (dict(dropout_keep=1.5), E_BADARG),
                       (dict(storage=3), E_BADARG)):
        d = make_desc(r, T.FP32S, **over)
        calls = [lambda: L.unetk_norm_drop_pool(ctypes.byref(d), _p(y), _p(st["mean"]), _p(st["rstd"]), _p(sums), _stream()),
                 lambda: L.unetk_norm_se_bwd_add_drop(ctypes.byref(d), _p(y), _p(dy), _p(st["mean"]), _p(st["rstd"]), _p(st["scale"]),
                                                      _p(st["A"]), _p(st["k1"]), _p(st["k2"]), _stream())]
        if "dropout_keep" not in over:
            calls.append(lambda: L.unetk_norm_se_bwd_add(ctypes.byref(d), _p(y), _p(dy), _p(st["mean"]), _p(st["rstd"]), _p(st["scale"]),
                                                         _p(st["A"]), _p(st["k2"]), _stream()))
        for fn in calls:
            rc, names = _trace(ops, fn)
            assert rc == code and names == [], (over, rc, names)
        assert sums.changed_anywhere() == 0 and dy.changed_anywhere() == 0
