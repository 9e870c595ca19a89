"""Non-finite values on the forward path (include/unetk.h): every kernel family against its row of tests/nonfinite_cases.py, and
whole networks with one poisoned element.

Op level.  A row puts a NaN (both bit patterns of nonfinite_cases.PAYLOADS) at one to three elements of one operand of an
existing exact-tier path row, runs the entry point the path test runs (its launch trace is asserted, so a row cannot drift to
another kernel) and asserts
  R <= isnan(result) <= A        (R: the in-image receptive field holds the poison; A: the same with the zero halo counted)
  outside A: the float64 result of the CLEAN inputs, bit for bit (bf16 storage: float64 rounded once).
Statistic partials of the conv rows, per (row, channel): the row of every output pixel comes from the candidate map that the
kernel's CLEAN partials fit against float64 (tiles of a plane, runs of a sample's pixels, the interleaved rows of the subsample
kernel); an entry is NaN if its pixels meet R and only if they meet A, in both sums, and every other entry equals the clean
launch bit for bit.  Concat neighbours of the transposed convs stay bit-equal.

End to end.  All networks run with weight_decay_rate = 0, so the L2 sum over the variables cannot be what carries a NaN to the
loss: it has to travel through the activations.  isnan(loss) must equal isnan(oracle loss) for a NaN input pixel, a +Inf input
pixel, a NaN decoder conv weight and a NaN encoder norm beta; in eval mode isnan(logits) must equal the oracle's element for
element.  The oracle (oracle/*.py, torch on the CPU: torch.relu and F.max_pool2d propagate NaN) was run on these very cases
without a device: UNet with batch norm, instance norm, --without_norm and bf16c operands, and UNet3D -- loss NaN for each of the
four poisons (healthy step: 1.3422, 1.3388, 1.1496, 1.3421, 1.5180), eval logits NaN on all 3072 (UNet) / 8192 (UNet3D)
elements of the poisoned sample and on none of the other.  GUNet's variables start from the device model's own initialisation,
so its oracle runs inside the test only; every test recomputes the oracle's answer and asserts that it is NaN where stated.

Not covered here: the backward kernels, which the contract leaves alone.
"""
import ctypes

import numpy as np
import pytest
import torch

import guardbuf
import nonfinite_cases as T
import norm_paths as NP
import small_ops_cases as S

pytestmark = pytest.mark.gpu

FP32, BF16, BF16S = T.FP32, T.BF16, T.BF16S


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
    return ctypes.c_void_p(t if isinstance(t, int) else (t.ptr() if hasattr(t, "ptr") else t.data_ptr()))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _norm_name(name):
    return name.replace(" ", "").replace("(anonymousnamespace)::", "")


def _trace(ops, fn):
    ops.profile_begin(0)
    ops.profile_on([])
    try:
        out = fn()
    finally:
        ops.profile_on(None)
    torch.cuda.synchronize()
    return out, [_norm_name(n) for n in ops.profile_read()[1] if "pack_" not in n]


def _assert_trace(names, expect, what):
    assert len(names) == len(expect) and all(e in g for e, g in zip(expect, names)), "{}: traced {} expected {}".format(what, names, expect)


def _sd(prec):
    return torch.bfloat16 if prec == BF16S else torch.float32


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dtype)


def _put(view, pos, k):
    """The k-th poison pattern at the elements `pos` of a device tensor (any strides), written as bits: no conversion touches it."""
    wide = view.dtype == torch.float32
    assert wide or view.dtype == torch.bfloat16, view.dtype
    pat = T.PAYLOADS[k][0 if wide else 1]
    bits = view.view(torch.int32 if wide else torch.int16)
    for p in pos:
        bits[p] = pat - (1 << (32 if wide else 16)) if pat >> (31 if wide else 15) else pat
    got = view[tuple(np.array(pos).T.tolist())] if len(pos) else view
    assert bool(torch.isnan(got.float()).all())


def _poison_guarded(g, pos, k):
    _put(g.view, pos, k)
    g.snap = g.flat.clone()                                      # the poison is part of the input from here on


def _check(what, got_t, R, A, clean, prec_out):
    got = got_t.float().cpu().numpy().astype(np.float64).reshape(R.shape)
    nan = np.isnan(got)
    assert not (R & ~nan).any(), "{}: {} of {} outputs that hold the poison are finite, first at {}".format(
        what, int((R & ~nan).sum()), int(R.sum()), np.argwhere(R & ~nan)[:3].tolist())
    assert not (nan & ~A).any(), "{}: {} outputs outside A are NaN, first at {}".format(what, int((nan & ~A).sum()),
                                                                                     np.argwhere(nan & ~A)[:3].tolist())
    want = T.stored(clean, prec_out)
    bad = (got != want) & ~A
    assert not bad.any(), "{}: {} clean outputs differ from float64, first at {}".format(what, int(bad.sum()), np.argwhere(bad)[:3].tolist())


def _row_maps(shape, rows, c):
    """Candidate maps from output pixel to statistic row for y [N, (D,) H, W, C] with `rows` rows, as int arrays over the pixels:
    h x w tiles of every plane in (plane, tile row, tile column) order; runs of bm consecutive pixels of a sample or of a plane;
    and the interleaved rows of subsample2_stats_kernel (rows / N blocks per sample, each taking every (rows / N)-th run of
    256 / (C / 4) pixels).  Which one a kernel uses is decided by its CLEAN partials against float64 (_check_stats)."""
    n, h, w = shape[0], shape[-3], shape[-2]
    d = shape[1] if len(shape) == 5 else 1
    planes = n * d
    hh, ww = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for th in range(1, max(h, 64) + 1):
        for tw in (4, 8, 12, 16, 32, 64):
            nth, ntw = -(-h // th), -(-w // tw)
            if (th <= h or th in (2, 4, 8, 16, 32, 64)) and planes * nth * ntw == rows:
                tile = (hh // th) * ntw + ww // tw
                yield "tiles %d x %d" % (th, tw), (np.arange(planes)[:, None, None] * (nth * ntw) + tile[None]).reshape(shape[:-1])
    for groups, what in ((n, "sample"), (planes, "plane")):
        if rows % groups == 0:
            per, pg = rows // groups, (planes // groups) * h * w
            for bm in (32, 64, 128, 256, 512, 1024):
                if -(-pg // bm) == per:
                    lin = np.arange(pg) // bm
                    yield "%d pixels of a %s" % (bm, what), (np.arange(groups)[:, None] * per + lin[None]).reshape(shape[:-1])
    if rows % n == 0 and c % 4 == 0:
        bps, rpi, pg = rows // n, 256 // (c // 4), d * h * w
        lin = (np.arange(pg) // rpi) % bps
        yield "interleaved", (np.arange(n)[:, None] * bps + lin[None]).reshape(shape[:-1])


def _by_row(rowof, rows, v):
    out = np.zeros((rows, v.shape[-1]), np.float64)
    np.add.at(out, rowof.reshape(-1), v.reshape(-1, v.shape[-1]).astype(np.float64))
    return out


def _check_stats(what, stats, stats_clean, R, A, y, lsb, atol_sum, rtol_sq):
    """Statistic partials [2][rows][C] of a conv, per (row, channel).  y: float64 of the clean inputs as the tensor stores it.
    The row of every output pixel is the candidate of _row_maps whose float64 sums the CLEAN device partials equal (bit for bit
    where the sums are exact in fp32 in any order, else at the family's bounds per entry); a row that fits no candidate fails.
    Then: an entry is NaN if its row's pixels meet R and only if they meet A, in both sums, and every other entry equals the
    clean run's bit for bit."""
    s, s0 = stats.double().cpu().numpy(), stats_clean.double().cpu().numpy()
    rows, c = s.shape[1], s.shape[2]
    assert np.isfinite(s0).all(), what
    fits = None
    for name, rowof in _row_maps(R.shape, rows, c):
        r1, r2, mag = _by_row(rowof, rows, y), _by_row(rowof, rows, y * y), _by_row(rowof, rows, np.abs(y))
        pix = np.bincount(rowof.reshape(-1), minlength=rows).max()
        ymax = np.abs(y).max()
        exact = lsb is not None and pix * ymax / lsb < 2 ** 24 and pix * ymax * ymax / (lsb * lsb) < 2 ** 24
        if exact:
            ok = np.array_equal(s0[0], r1) and np.array_equal(s0[1], r2)
        else:
            ok = (np.abs(s0[0] - r1) <= atol_sum * np.maximum(1.0, mag)).all() and (np.abs(s0[1] - r2) <= rtol_sq * r2 + 1e-30).all()
        if ok:
            fits = (name, rowof, exact)
            break
    assert fits is not None, what + ": the clean statistic partials fit no row map (%d rows)" % rows
    name, rowof, exact = fits
    print(what, "statistic rows:", name, "exact" if exact else "bounds")
    row_r = _by_row(rowof, rows, R) > 0
    row_a = _by_row(rowof, rows, A) > 0
    assert row_r.any(), what
    nan = np.isnan(s)
    for k in (0, 1):
        assert not (row_r & ~nan[k]).any(), "{}: sum {}: {} (row, channel) entries whose pixels hold the poison are finite, first {}".format(
            what, k, int((row_r & ~nan[k]).sum()), np.argwhere(row_r & ~nan[k])[:3].tolist())
        assert not (nan[k] & ~row_a).any(), "{}: sum {}: {} clean (row, channel) entries are NaN, first {}".format(
            what, k, int((nan[k] & ~row_a).sum()), np.argwhere(nan[k] & ~row_a)[:3].tolist())
        keep = ~nan[k]
        assert np.array_equal(s[k][keep], s0[k][keep]), what + ": sum %d: a clean (row, channel) entry moved" % k


def _params(fam):
    return [pytest.param(r.id, k, id="%s-p%d" % (r.id, k)) for r in T.rows(fam) for k in (0, 1)]


# ------------------------------------------------------------------ pools and the context branch
@pytest.mark.parametrize("rid,k", _params("mp2"))
def test_maxpool2_window_with_a_nan_is_nan(ops, rid, k):
    row = T.BY_ID[rid]
    c = T.case(row)
    p = c["src"].p
    sd = _sd(row.prec)
    gx = guardbuf.guarded_input(_dev(c["inputs"]["x"], sd), p["xs"], p["xo"])
    _poison_guarded(gx, row.pos, k)
    out, names = _trace(ops, lambda: ops.maxpool2_fwd(gx.view))
    _assert_trace(names, ["maxpool2_fwd_kernel<%s>" % ("unsignedshort" if row.prec == BF16S else "float")], rid)
    assert gx.changed_anywhere() == 0
    _check(rid, out, *c["outs"]["p"], row.prec)


@pytest.mark.parametrize("rid,k", _params("mp1"))
def test_maxpool1d_window_with_a_nan_is_nan(ops, rid, k):
    row = T.BY_ID[rid]
    c = T.case(row)
    p = c["src"].p
    x = _dev(c["inputs"]["x"])
    _put(x, row.pos, k)
    y = torch.full((p["b"], (p["l"] + 1) // 2, p["c"]), 7.0, device="cuda")
    rc, names = _trace(ops, lambda: lib().unetk_maxpool1d_fwd(_p(x), _p(y), p["b"], p["l"], p["c"], _stream()))
    assert rc == 0
    _assert_trace(names, ["maxpool1d_fwd_kernel"], rid)
    _check(rid, y, *c["outs"]["y"], FP32)


@pytest.mark.parametrize("rid,k", _params("avg") + _params("smean") + _params("moments"))
def test_averaging_kernels_give_nan_by_arithmetic(ops, rid, k):
    row = T.BY_ID[rid]
    c = T.case(row)
    p = c["src"].p
    name = T.MAIN[row.fam]
    x = _dev(c["inputs"][row.operand])
    _put(x, row.pos, k)
    if row.fam == "avg":
        out, names = _trace(ops, lambda: ops.avgpool2_fwd(x))
        expect = ["avgpool2_fwd_kernel"]
    elif row.fam == "smean":
        out = torch.full((p["n"], p["c"]), 7.0, device="cuda")
        rc, names = _trace(ops, lambda: lib().unetk_spatial_mean_fwd(_p(x), _p(out), p["n"], p["hw"], p["c"], _stream()))
        assert rc == 0
        expect = ["spatial_mean_fwd_kernel"]
    else:
        g = p["g"]
        out = torch.full((p["n"] if p["ps"] else 1, g + g * g), 7.0, device="cuda")
        rc, names = _trace(ops, lambda: lib().unetk_guide_moments(_p(x), p["n"], p["hw"], g, p["ps"], _p(out), _stream()))
        assert rc == 0
        expect = ["guide_moments_kernel"]
    _assert_trace(names, expect, rid)
    _check(rid, out, *c["outs"][name], FP32)


@pytest.mark.parametrize("rid,k", _params("fc") + _params("conv1d"))
def test_fc_and_conv1d_forward(ops, rid, k):
    row = T.BY_ID[rid]
    c = T.case(row)
    p, a = c["src"].p, c["inputs"]
    t = {n: (_dev(a[n]) if a.get(n) is not None else None) for n in ("x", "w", "b")}
    _put(t[row.operand], row.pos, k)
    if row.fam == "fc":
        y = torch.full((p["b"], p["n"]), 7.0, device="cuda")
        mask = torch.full((p["b"], p["n"]), 7.0, device="cuda") if p["keep"] is not None else None
        keep = p["keep"] if p["keep"] is not None else 1.0
        rc, names = _trace(ops, lambda: lib().unetk_fc_fwd(_p(t["x"]), _p(t["w"]), _p(t["b"]), _p(y), _p(mask), p["b"], p["k"], p["n"],
                                                          p["relu"], keep, S.SEED, _stream()))
        expect = ["fc_fwd_kernel"]
        if mask is not None:                                      # the dropped units of test_nonfinite_host.py are the device's
            assert np.array_equal(mask.cpu().numpy().astype(np.float64), a["mask"])
    else:
        y = torch.full((p["b"], p["l"], p["co"]), 7.0, device="cuda")
        rc, names = _trace(ops, lambda: lib().unetk_conv1d_fwd(_p(t["x"]), _p(t["w"]), _p(t["b"]), _p(y), p["b"], p["l"], p["ci"], p["co"],
                                                              p["k"], p["relu"], _stream()))
        expect = ["conv1d_fwd_kernel"]
    assert rc == 0
    _assert_trace(names, expect, rid)
    _check(rid, y, *c["outs"]["y"], FP32)


# ------------------------------------------------------------------ norm apply + ReLU (+ pool)
@pytest.mark.parametrize("rid,k", _params("norm") + _params("normpool"))
def test_norm_apply_relu_passes_nan_on(ops, rid, k):
    import test_gpu_norm_paths as NG
    row = T.BY_ID[rid]
    c = T.case(row)
    r, st = c["src"], c["storage"]
    call = NG.Call(r, st, c["inputs"])
    if row.operand == "gw":                                       # [Ng, G, gw_stride], the data at columns gw_coff ..
        _put(call.gw, [(a, b, r.coff + ch) for a, b, ch in row.pos], k)
    else:
        g = {"y": call.y, "scale": call.stat[0], "shift": call.stat[1], "den": call.den}[row.operand]
        _poison_guarded(g, row.pos, k)
    rc, names = _trace(ops, call.apply)
    assert rc == 0, rc
    _assert_trace(names, NP.expected_apply(r, st), rid)
    outs = [call.z] + ([call.pooled] if r.kind == "pool" else [])
    call.check_guards(rid, outs)
    _check(rid + " z", call.z.view, *c["outs"]["z"], row.prec)
    if r.kind == "pool":
        _check(rid + " pooled", call.pooled.view, *c["outs"]["pooled"], row.prec)


@pytest.mark.parametrize("which", ["both", "sum_y", "sum_y2"])
@pytest.mark.parametrize("per_sample", [False, True], ids=["batch_norm", "instance_norm"])
@pytest.mark.parametrize("k", [0, 1])
def test_norm_finalize_carries_nan_statistics_into_mean_rstd_scale_shift_and_moving_statistics(ops, per_sample, k, which):
    """NaN statistic partials of one (row, channel).  `both` is what one NaN or Inf conv output leaves (sum y and sum y^2): mean,
    rstd, scale and shift of that (group, channel) are NaN and, under batch norm in training, the channel's moving mean AND
    moving variance.  `sum_y` alone gives the same (the variance subtracts mean^2); `sum_y2` alone leaves the mean and the moving
    mean finite.  Every other entry equals the clean call bit for bit (that call is pinned by tests/test_gpu_norm_stats.py)."""
    n, hw, c, rows = 3, 40, 24, 6
    rng = np.random.default_rng(5)
    y = rng.integers(-4, 5, (n, rows // n, hw // (rows // n), c)).astype(np.float64)          # rows: two per sample
    part = np.stack([y.sum(2), (y * y).sum(2)]).reshape(2, rows, c)
    gamma, beta = _dev(rng.integers(1, 4, c) / 2.0), _dev(rng.integers(-8, 9, c) / 8.0)
    d = ops.norm_desc((n, hw, c), per_sample)
    sums = {"both": (0, 1), "sum_y": (0,), "sum_y2": (1,)}[which]

    def run(poison):
        stats = _dev(part)
        if poison:
            _put(stats, [(q, 3, 7) for q in sums], k)             # the second row of sample 1, channel 7
        mm, mv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        out = ops.norm_finalize(d, stats, rows, gamma, beta, 1e-3, 0.999, True, None if per_sample else mm, None if per_sample else mv, gamma.device)
        torch.cuda.synchronize()
        return out.clone(), mm, mv
    clean, mm0, mv0 = run(False)
    got, mm1, mv1 = run(True)
    assert bool(torch.isfinite(clean).all())
    want = torch.zeros_like(got, dtype=torch.bool)                # [mean, rstd, scale, shift][group][channel]
    want[(0 if 0 in sums else 1):, 1 if per_sample else 0, 7] = True
    assert torch.equal(torch.isnan(got), want), torch.isnan(got).nonzero().tolist()
    assert torch.equal(got[~want].view(torch.int32), clean[~want].view(torch.int32))
    if not per_sample:
        only7 = [ch == 7 for ch in range(c)]
        assert torch.isnan(mv1).tolist() == only7
        assert torch.isnan(mm1).tolist() == (only7 if 0 in sums else [False] * c)
        keep = ~torch.tensor(only7, device="cuda")
        assert torch.equal(mv1[keep], mv0[keep]) and torch.equal(mm1[keep], mm0[keep])
        if 0 not in sums:
            assert torch.equal(mm1, mm0)


# ------------------------------------------------------------------ conv3x3 forward with statistics, fused epilogues
def _conv_operands(ops, c, row, k, cin, cout, poison=True):
    """Device x (fp32, or bf16 under bf16 storage behind the first layer) and the filter as the entry point wants it, poisoned
    (poison=False: the clean operands, for the clean statistic partials)."""
    first = not (cin % 16 == 0 and cout % 32 == 0)
    x = _dev(c["inputs"]["x"], torch.float32 if first else _sd(row.prec))
    w = _dev(c["inputs"]["w"])
    if poison and row.operand == "x":
        _put(x, row.pos, k)
    elif poison and row.operand == "w":
        _put(w, row.pos, k)
    wsrc = w if first else ops.conv3x3_pack(w, want_dgrad=False, bf16=row.prec)[0]
    return x, wsrc


@pytest.mark.parametrize("rid,k", _params("conv"))
def test_conv3x3_forward_and_statistics(ops, rid, k):
    row = T.BY_ID[rid]
    c = T.case(row)
    case = c["src"]
    e_fwd, e_rows = {FP32: (case.fwd, case.rows), BF16: (case.bf16 or (None,) * 2)[:2], BF16S: (case.bf16s or (None,) * 2)[:2]}[row.prec]
    assert e_fwd is not None, rid
    x, wsrc = _conv_operands(ops, c, row, k, case.cin, case.cout)
    (y, stats, rows), names = _trace(ops, lambda: ops.conv3x3_fwd(x, wsrc, case.cout, True, bf16=row.prec, dilation=case.dil))
    _assert_trace(names, e_fwd, rid)
    assert rows == e_rows and tuple(stats.shape) == (2, rows, case.cout)
    R, A, clean = c["outs"]["y"]
    _check(rid, y, R, A, clean, row.prec)
    x0, w0 = _conv_operands(ops, c, row, k, case.cin, case.cout, poison=False)
    y0, stats0, _ = ops.conv3x3_fwd(x0, w0, case.cout, True, bf16=row.prec, dilation=case.dil)
    assert np.array_equal(y0.float().cpu().numpy().astype(np.float64), T.stored(clean, row.prec)), rid + ": the clean run"
    # (conv3x3_igemm_bf16_kernel under bf16 storage sums its fp32 accumulators, not the rounded values it stores: float64 as it
    # is.)  Bounds where the sums are not exact: test_gpu_conv_paths.py's, per entry
    _check_stats(rid, stats, stats0, R, A, clean, c["lsb"], 2e-4, 2e-5)


@pytest.mark.parametrize("rid,k", _params("aff"))
def test_fused_epilogues_relu_and_pool(ops, rid, k):
    import test_gpu_conv_epilogue_paths as EP
    row = T.BY_ID[rid]
    c = T.case(row)
    r, pool = c["src"], row.opt["pool"]
    assert r.prec == row.prec and ops.conv3x3_fwd_affine_ok(r.n, r.h, r.w, r.cin, r.cout, pool=pool, bf16=row.prec), rid
    x, wsrc = _conv_operands(ops, c, row, k, r.cin, r.cout)
    scale, shift = _dev(c["inputs"]["scale"]), _dev(c["inputs"]["shift"])
    if row.operand in ("scale", "shift"):
        _put(scale if row.operand == "scale" else shift, row.pos, k)
    (z, pooled), names = _trace(ops, lambda: ops.conv3x3_fwd_affine(x, wsrc, r.cout, scale, shift, pool=pool, bf16=row.prec))
    expect = [kn.format(m=(2 if pool else 1) if kn.startswith(EP.V3) else (4 if pool else 3)) for kn in r.kern]
    _assert_trace(names, expect, rid)
    _check(rid + " z", z, *c["outs"]["z"], row.prec)
    if pool:
        _check(rid + " pooled", pooled, *c["outs"]["pooled"], row.prec)


# ------------------------------------------------------------------ transposed convs: bias + ReLU into a concat slice
@pytest.mark.parametrize("rid,k", _params("deconv"))
def test_deconv_forward_and_concat_neighbours(ops, rid, k):
    import test_gpu_deconv_paths as DP
    row = T.BY_ID[rid]
    c = T.case(row)
    r, a = c["src"], c["inputs"]
    assert DP.fwd_ok(r, row.prec), rid
    f32 = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32))
    call = DP.Call(r, row.prec, f32(a["x"]), f32(a["w"]), f32(a["b"]), c["dup"])
    if row.operand == "x":
        _poison_guarded(call.gx, row.pos, k)
    elif row.operand == "w":
        _put(call.wg, row.pos, k)
    else:
        _poison_guarded(call.bg, row.pos, k)
    assert call.pack() == 0
    torch.cuda.synchronize()
    rc, names = _trace(ops, call.fwd)
    assert rc == 0, rc
    _assert_trace(names, DP.expected(r, row.prec)[0], rid)
    assert call.gcat.changed_outside() == 0, rid + ": a neighbouring concat channel or a guard changed"
    assert call.gcat.unwritten() == 0 and call.gx.changed_anywhere() == 0
    _check(rid, call.gcat.view, *c["outs"]["up"], row.prec)


# ------------------------------------------------------------------ conv3d forward with statistics
@pytest.mark.parametrize("rid,k", _params("conv3d"))
def test_conv3d_forward_and_statistics(ops, rid, k):
    import test_gpu_ops3d as O3
    row = T.BY_ID[rid]
    c = T.case(row)
    n, dd, h, w, cin, cout, kd, stride = c["geom"]
    live8 = None if c["live"] is None else (O3._mask8(c["live"][0]), O3._mask8(c["live"][1]))
    x, wt = _dev(c["inputs"]["x"]), _dev(c["inputs"]["w"])
    _put(x if row.operand == "x" else wt, row.pos, k)
    d = ops.conv3d_desc(tuple(x.shape), cout, kd, stride, live8=live8)
    wp_f, _ = ops.conv3d_pack(wt, want_dgrad=False, precision=row.prec)
    torch.cuda.synchronize()
    (y, stats, rows), names = O3._trace(ops, lambda: ops.conv3d_fwd(x, wp_f, d, want_stats=True, precision=row.prec))
    assert len(names) == len(c["trace"]) and all(e in g for e, g in zip(c["trace"], names)), (rid, names, c["trace"])
    R, A, clean = c["outs"]["y"]
    _check(rid, y, R, A, clean, FP32)
    x0, w0 = _dev(c["inputs"]["x"]), _dev(c["inputs"]["w"])
    y0, stats0, _ = ops.conv3d_fwd(x0, ops.conv3d_pack(w0, want_dgrad=False, precision=row.prec)[0], d, want_stats=True, precision=row.prec)
    assert np.array_equal(y0.cpu().numpy().astype(np.float64), clean), rid + ": the clean run"
    # x integers, w eighths: exact sums wherever a row's pixels stay below 2^24 units (as the 2-D rows); else the bounds of
    # test_gpu_ops3d.py::test_conv3d_forward_backward, per entry
    _check_stats(rid, stats, stats0, R, A, clean, 0.125, 3e-4, 3e-5)


# ------------------------------------------------------------------ whole networks: a poisoned step is refused
NETS = ["unet_bn", "unet_in", "unet_nonorm", "unet_bf16c", "gunet_guide", "unet3d", "unet3d_bf16c"]
POISONS = ["nan_pixel", "inf_pixel", "nan_decoder_weight", "nan_encoder_beta"]
_NETS = {}


def _unet(**over):
    import test_gpu_unet as t
    from oracle import unet2d
    args = t.make_args(weight_decay_rate=0.0, **over)
    images, labels = t.synth(2, 32, 32, 3)
    model, inputs = t.build(args, images, labels)
    net = unet2d.UNet2DOracle(3, 3, init_channels=64, num_down_samples=4, normalizer=args.normalizer, without_norm=args.without_norm)
    if getattr(args, "compute_dtype", "fp32") == "bf16c":
        net.bf16 = 1
    params = unet2d.init_params(net.specs, seed=77)
    g = torch.Generator().manual_seed(5)
    for name, _, kind in net.specs:
        if kind == "gamma":
            params[name] = 0.5 + torch.rand(params[name].shape, generator=g)
        elif kind in ("beta", "bias"):
            params[name] = 0.2 * torch.randn(params[name].shape, generator=g)
    kw = t.loss_kwargs(args)
    beta = "UNet/Encode1/Repeat/convolution2d_1/" + ("biases" if args.without_norm else
                                                    ("BatchNorm" if args.normalizer == "batch_norm" else "InstanceNorm") + "/beta")
    return dict(model=model, inputs=inputs, yml=t.YML, params=params, image=torch.from_numpy(images), pixel=(1, 10, 12, 1),
                decoder_w="UNet/Decode2/Repeat/convolution2d_1/weights", beta=beta,
                oracle_loss=lambda p, im: net.loss(p, im, torch.from_numpy(labels).long(), **kw)[0],
                oracle_logits=lambda p, im: net.forward(p, im, False)[0])


def _gunet():
    import test_gpu_gunet as G
    args = G.make_args(weight_decay_rate=0.0)
    model, inputs, net, params, (images, guide, labels) = G.setup(args)
    kw = G.kwargs_of(args)
    return dict(model=model, inputs=inputs, yml=G.YML, params=params, image=images, pixel=(1, 10, 12, 1),
                decoder_w="GUNet/Decode/up_conv2/up_conv2_1/weights", beta="GUNet/Encode/down_conv1/mod_conv1/InstanceNorm/beta",
                oracle_loss=lambda p, im: net.loss(p, im, guide, labels, **kw)[0],
                oracle_logits=lambda p, im: net.forward(p, im, guide, False)[0])


def _unet3d(bf16c):
    import test_gpu_unet3d as U
    args = U.make_args(weight_decay_rate=0.0, **(dict(compute_dtype="bf16c") if bf16c else {}))
    model, inputs, net, params, (images, labels) = U.setup(args)
    kw = U.kwargs_of(args)
    # the oracle of the bf16c net is the same restatement: rounding the conv operands to bf16 moves no NaN and makes none
    return dict(model=model, inputs=inputs, yml=U.YML, params=params, image=images, pixel=(1, 2, 10, 12, 0),
                decoder_w="UNet3D/conv_d1/conv1/weights", beta="UNet3D/conv_e0/conv1/InstanceNorm/beta",
                oracle_loss=lambda p, im: net.loss(p, im, labels, **kw)[0],
                oracle_logits=lambda p, im: net.forward(p, im, False)[0])


def _net(name):
    if name not in _NETS:
        _NETS.clear()                                             # one network's buffers at a time
        _NETS[name] = {"unet_bn": lambda: _unet(), "unet_in": lambda: _unet(normalizer="instance_norm"),
                       "unet_nonorm": lambda: _unet(without_norm=True), "unet_bf16c": lambda: _unet(compute_dtype="bf16c"),
                       "gunet_guide": _gunet, "unet3d": lambda: _unet3d(False), "unet3d_bf16c": lambda: _unet3d(True)}[name]()
    return _NETS[name]


def _poisoned_net(s, poison):
    """(variables, image batch) of one poison: a single element differs from the healthy step."""
    params = {n: v.clone() for n, v in s["params"].items()}
    image = s["image"].clone()
    if poison == "nan_pixel":
        image[s["pixel"]] = float("nan")
    elif poison == "inf_pixel":
        image[s["pixel"]] = float("inf")
    elif poison == "nan_decoder_weight":
        params[s["decoder_w"]].view(-1)[3] = float("nan")
    elif poison == "nan_encoder_beta":
        params[s["beta"]].view(-1)[3] = float("nan")
    else:
        assert poison == "none", poison
    return params, image


def _device_inputs(s, image):
    inputs = dict(s["inputs"])
    inputs["images"] = image.cuda()
    return inputs


@pytest.mark.parametrize("poison", POISONS + ["none"])
@pytest.mark.parametrize("name", NETS)
def test_poisoned_training_step_has_a_nan_loss_like_the_oracle(name, poison):
    """weight_decay_rate = 0: the NaN can reach the loss through the network only.  The oracle's loss is NaN for each of the four
    poisons on each of the seven networks (recorded from a CPU run of these cases) and finite for the healthy step."""
    s = _net(name)
    params, image = _poisoned_net(s, poison)
    with torch.no_grad():
        ref = float(s["oracle_loss"](params, image))
    assert np.isnan(ref) == (poison != "none"), (name, poison, ref)
    s["model"].params.load_state(params)
    got = float(s["model"](_device_inputs(s, image), "train", **s["yml"]).item())
    print(name, poison, "loss", got, "oracle", ref)
    assert np.isnan(got) == np.isnan(ref), (name, poison, got, ref)


@pytest.mark.parametrize("name", NETS)
def test_eval_logits_are_nan_where_the_oracles_are(name):
    """Eval mode (moving statistics under batch norm) with a NaN input pixel: the NaN pattern of the logits equals the oracle's
    element for element -- the poisoned sample, and no element of the other one."""
    s = _net(name)
    params, image = _poisoned_net(s, "nan_pixel")
    with torch.no_grad():
        ref = torch.isnan(s["oracle_logits"](params, image))
    assert bool(ref.any()) and not bool(ref.all())
    s["model"].params.load_state(params)
    s["model"](_device_inputs(s, image), "eval", **s["yml"])
    got = torch.isnan(s["model"].layers["logits"]).cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got, ref), (name, int(got.sum()), int(ref.sum()), int((got != ref).sum()))
