"""No GPU: the table of tests/test_gpu_norm_paths.py is self-consistent.

Every row's hand-written kernel names and reducer launches agree with a Python restatement of norm.hip's host code (geom,
unetk_colmap, bwd_blocks, the apply grid, unetk_rows_reduce_alias' row thresholds); every branch the file exists to reach is taken
by at least one row and every cap has a row at it and one over it; every value the exact tier compares bit for bit is
float32-representable and every sum stays under 2^24 units; the closed-form backward of oracle/norm_unit.py equals float64
autograd where the given statistics are the true ones.
"""
import numpy as np
import pytest
import torch

import norm_paths as T
from oracle import norm_unit, tf_ops

UNIT = [r for r in T.ROWS if r.kind == "unit"]
POOL = [r for r in T.ROWS if r.kind == "pool"]
SE = [r for r in T.ROWS if r.kind == "se"]
PLANS = {r.id: T.plan(r) for r in T.ROWS}


def _tmpl(r):
    return "%d,%s,%s" % (r.g, "true" if r.den else "false", "true" if r.leaky else "false")


def test_rows_name_what_the_dispatch_code_launches():
    for r in T.ROWS:
        assert r.c % 4 == 0 and 4 <= r.c <= 1024
        p = PLANS[r.id]
        assert p["lds"] <= 64 << 10 and p["cq_n"] * p["rpi"] <= 256 and p["rpi"] >= 1, r.id
        if r.kind == "se":
            continue
        assert list(r.red) == p["red"], (r.id, r.red, p["red"])
        if r.kind == "unit":
            assert r.tmpl == _tmpl(r), (r.id, r.tmpl, _tmpl(r))
            # what the entry points admit
            assert not (r.leaky and r.g < 1) and not (r.leaky == 3 and not r.den) and not (r.gps and p["L"] != r.n)
            assert not (r.keep and (r.g or r.gbare) and not r.den and not r.leaky)
            if r.pre:
                assert r.tmpl == T.PLAIN and not (r.gbare or r.keep or r.affine) and r.pre % p["L"] == 0
        else:
            assert r.w % 2 == 0 and r.hw % r.w == 0 and (r.hw // r.w) % 2 == 0 and not (r.g or r.den or r.keep)
        assert T.ws_bytes(r) >= 4 * (p["K"] * p["L"] * p["nblk"] * r.c + p["K"] * p["L"] * r.c + p["K"] * r.c +
                                     T.tmp_floats(p["K"] * p["L"], T.RR_DIRECT_ROWS + 1, r.c)), r.id


def _some(pred, rows=T.ROWS):
    return [r.id for r in rows if pred(r, PLANS[r.id])]


def test_every_listed_branch_has_a_row():
    # thread map: idle threads 4 / 16 / 127 / 6 at C = 24 / 96 / 516 / 1000, C = 4 (one quad, 256 row lanes)
    for c, cq, rpi, idle in ((24, 6, 42, 4), (96, 24, 10, 16), (516, 129, 1, 127), (1000, 250, 1, 6), (4, 1, 256, 0), (200, 50, 5, 6)):
        assert T.colmap(c) == (cq, rpi) and 256 - cq * rpi == idle
        for ps in (0, 1):
            assert _some(lambda r, p: r.c == c and r.ps == ps and r.kind == "unit"), (c, ps)
    for c in (96, 516):
        for ps in (0, 1):
            assert _some(lambda r, p: r.c == c and r.ps == ps and r.g == 2 and r.den and r.bf)
    # template switch, both storages
    for g in range(5):
        for den, leaky in ((False, 0), (True, 0), (False, 2), (True, 2), (True, 3)):
            if leaky and not g:
                continue
            assert _some(lambda r, p: r.g == g and r.den == den and r.leaky == leaky and r.bf, UNIT), (g, den, leaky)
    assert _some(lambda r, p: r.leaky == 1 and r.den, UNIT) and _some(lambda r, p: r.leaky == 1 and not r.den, UNIT)
    assert _some(lambda r, p: r.affine and p["L"] == 1) and _some(lambda r, p: r.affine and p["L"] > 1)
    # dy bit for bit (xdy) in every template family, plain and with dropout, both storages; the affine path; the pool kernels
    for den, leaky in ((False, 0), (True, 0), (False, 2), (True, 2), (True, 3)):
        for drop in (False, True):
            assert _some(lambda r, p: r.xdy and r.bf and r.den == den and r.leaky == leaky and bool(r.keep) == drop and
                         (r.g > 0 or not leaky), UNIT), (den, leaky, drop)
    for ps in (0, 1):
        assert _some(lambda r, p: r.xdy and r.bf and r.affine and r.ps == ps, UNIT)
        assert _some(lambda r, p: r.xdy and r.bf and r.ps == ps, POOL)
    assert _some(lambda r, p: r.xdy and r.gps and r.leaky == 3) and _some(lambda r, p: r.xdy and r.pre and r.prealign)
    assert _some(lambda r, p: r.xdy and r.pre and not r.prealign)
    assert _some(lambda r, p: r.gps and r.n == 3 and not (r.den or r.leaky))                  # kb = 0
    assert _some(lambda r, p: r.gps and r.n == 3 and r.den and not r.ps)                      # kb = 2 + G, batch statistics
    assert _some(lambda r, p: r.gps and r.leaky == 3) and _some(lambda r, p: not r.gps and r.leaky == 3)    # post block groups N / 1
    assert _some(lambda r, p: r.coff > 0 and r.gstride > r.coff + r.c) and _some(lambda r, p: r.zpad and r.dzpad)
    assert _some(lambda r, p: r.gbare and not r.den and not r.g) and _some(lambda r, p: r.gbare and r.den)
    for keep in (0.5, 0.25):
        assert _some(lambda r, p: r.keep == keep, UNIT)
    # row-group tails: P in {1, rpi - 1, rpi, 4 rpi - 1, 4 rpi + 1} for the apply passes, 2 rpi -/+ 1 for the reduction
    for c in (64, 24):
        rpi = T.colmap(c)[1]
        for pp in (1, rpi - 1, rpi, T.GROUPS * rpi - 1, T.GROUPS * rpi + 1, T.RGROUPS * rpi - 1, T.RGROUPS * rpi + 1):
            assert _some(lambda r, p: r.c == c and p["P"] == pp and r.tmpl == T.PLAIN and not r.keep, UNIT), (c, pp)
    # grid caps: at the cap and one block over it
    row_groups = lambda r, p: T._cd(p["Q"], p["rpi"])
    assert _some(lambda r, p: p["L"] == 1 and row_groups(r, p) == 1024 and r.kind == "unit")
    assert _some(lambda r, p: p["L"] == 1 and row_groups(r, p) == 1025 and r.kind == "unit")
    assert _some(lambda r, p: p["L"] == 2 and p["nblk"] == 1024 and row_groups(r, p) == 1025)
    assert _some(lambda r, p: p["L"] == 40 and p["nblk"] == 64 and row_groups(r, p) == 64)
    assert _some(lambda r, p: p["L"] == 40 and p["nblk"] == 64 and row_groups(r, p) == 65)
    assert _some(lambda r, p: p["L"] == 1 and p["gx"] == 4096 and row_groups(r, p) == 4096, UNIT)
    assert _some(lambda r, p: p["L"] == 1 and p["gx"] == 4096 and row_groups(r, p) == 4097, UNIT)
    assert _some(lambda r, p: p["L"] == 3 and p["gx"] == 1366 and row_groups(r, p) == 1367, UNIT)
    assert _some(lambda r, p: p["nblk"] == 1024 and row_groups(r, p) == 1024, POOL)
    assert _some(lambda r, p: p["nblk"] == 1024 and row_groups(r, p) == 1025 and p["L"] == 1, POOL)
    assert _some(lambda r, p: p["nblk"] == 1024 and row_groups(r, p) == 1025 and p["L"] == 2, POOL)
    assert _some(lambda r, p: p["L"] == 1 and p["gx"] == 4096 and row_groups(r, p) == 4096, POOL)
    assert _some(lambda r, p: p["L"] == 1 and p["gx"] == 4096 and row_groups(r, p) == 4097, POOL)
    assert _some(lambda r, p: p["gx"] == 4096 and row_groups(r, p) == 4097, SE)
    assert _some(lambda r, p: p["L"] == 5 and p["gx"] == 820 and row_groups(r, p) == 821, SE)
    # reducer routes
    for nblk in (256, 257, 1024):
        assert _some(lambda r, p: not r.pre and p["nblk"] == nblk and p["L"] == 1, UNIT), nblk
    for k in (1, 256, 257, 1024, 1025):
        assert _some(lambda r, p: r.pre == k and p["L"] == 1 and r.prealign), k
    assert _some(lambda r, p: r.pre and p["L"] > 1 and r.pre // p["L"] > 1 and p["red"] == ["w", "w"])
    assert _some(lambda r, p: r.pre and p["red"] == ["l1", "w", "w"]) and _some(lambda r, p: p["red"] == ["l1", "n"])
    assert _some(lambda r, p: p["red"] == ["n"])
    assert _some(lambda r, p: r.den and not r.ps and r.n == 3 and r.g == 0)                  # second level into psum, batch norm + density
    simple = lambda r: r.tmpl == T.PLAIN and not r.gbare and r.kind == "unit"
    assert _some(lambda r, p: simple(r) and p["L"] == 1) and _some(lambda r, p: simple(r) and p["L"] > 1)
    # ksum / kst / krow: per-sample statistics; one group; batch statistics over several launch groups
    assert _some(lambda r, p: r.ps, UNIT) and _some(lambda r, p: not r.ps and p["L"] == 1, UNIT)
    assert _some(lambda r, p: not r.ps and p["L"] > 1, UNIT)
    # pool: one window; 2 x 6 and 6 x 2 planes; img = q / per_img (batch norm, N = 3) and img = n; a dskip stride > C
    assert _some(lambda r, p: r.hw == 4 and r.w == 2, POOL)
    assert _some(lambda r, p: r.w == 6 and r.hw == 12 and r.n == 3 and not r.ps, POOL)
    assert _some(lambda r, p: r.w == 2 and r.hw == 12 and r.n == 3 and r.ps, POOL)
    assert _some(lambda r, p: r.dzpad and r.bf, POOL)
    # one block per sample: N = 1 and 5, HW = 1 and 3, C = 24 and 1024
    for n in (1, 5):
        for hw in (1, 3):
            for c in (24, 1024):
                assert _some(lambda r, p: (r.n, r.hw, r.c) == (n, hw, c) and r.bf, SE)
    assert _some(lambda r, p: r.ps, SE) and _some(lambda r, p: not r.ps, SE)


def _check_unit_exact(r, ref, what):
    assert T.is_f32(ref["z"]), what
    for name, terms in ref["terms"].items():
        axes = (1,) if name == "dden" or (r.gps and name in ("dgw", "dgb", "dps")) else (0, 1)
        assert T.sum_exact(terms, axes), (what, name)
    if r.xdy:
        ps = PLANS[r.id]["Ps"]
        assert ps & (ps - 1) == 0, (what, ps)
        for step in ref["dy_steps"] + [ref["dy"]]:
            assert T.is_f32(step), what


@pytest.mark.parametrize("rid", [r.id for r in T.ROWS])
def test_exact_tier_values_are_representable_and_sums_stay_under_2_pow_24(rid):
    r = T.BY_ID[rid]
    for storage in (T.FP32S, T.BF16S) if r.bf else (T.FP32S,):
        a = T.make_inputs(r, "exact", storage)
        for k in ("y", "dz", "dp"):
            if k in a:
                assert np.array_equal(T.round_bf16(a[k]), a[k]), (rid, k)          # the stored tensors are exact in bf16
        for k in ("mean", "rstd", "scale", "shift", "den", "gw", "gb", "guide"):
            assert a[k] is None or T.is_f32(a[k]), (rid, k)
        if r.kind == "unit":
            ref = T.unit_reference(r, a)
            if T.exact_tier_is_bitwise(r):
                _check_unit_exact(r, ref, rid)
                if r.pre:
                    assert T.is_f32(T.pre_partials(r, ref))
            u0 = ref["u"] == 0
            if r.n * r.hw >= 8:
                assert (u0 & (np.asarray(a["dz"]) != 0)).any(), rid                 # ReLU ties under a non-zero gradient
        elif r.kind == "pool":
            ref = T.pool_reference(r, a, storage)
            _check_unit_exact(r, ref, rid)
            assert T.is_f32(ref["dz"]) and T.is_f32(ref["pooled"])
            n, h, w = r.n, r.hw // r.w, r.w
            z_st = ref["z"] if storage == T.FP32S else T.round_bf16(ref["z"])
            win = norm_unit.window_view(z_st, n, h, w)
            if r.hw >= 64:
                arg = win.argmax(3)
                assert set(np.unique(arg)) == {0, 1, 2, 3}, rid                     # a maximum at each of the four places
                assert (win.max(3) == win.min(3)).any(), rid                        # windows of four equal values
            if storage == T.BF16S and r.hw >= 12:
                w32 = norm_unit.window_view(ref["z"], n, h, w)
                tie_only_rounded = (np.sort(win, 3)[..., -1, :] == np.sort(win, 3)[..., -2, :]) & \
                                   (np.sort(w32, 3)[..., -1, :] != np.sort(w32, 3)[..., -2, :])
                assert tie_only_rounded.any(), rid
        else:
            ps = bool(r.ps)
            dy0 = np.asarray(a["dz"])
            assert T.is_f32(norm_unit.se_add(a["y"], dy0, a["mean"], a["rstd"], a["scale"], a["A"], a["k2"], ps))
            assert T.is_f32(norm_unit.se_add_drop(a["y"], dy0, a["mean"], a["rstd"], a["scale"], a["A"], a["k1"], a["k2"], a["mask"], ps))
            sums, terms = norm_unit.drop_pool(a["y"], a["mean"], a["rstd"], a["mask"], ps)
            assert T.sum_exact(terms["mx"], (1,)) and T.sum_exact(terms["m"], (1,)) and T.is_f32(sums)


def test_dropout_mask_restatement_keeps_its_share():
    for keep in (0.5, 0.25):
        m = T.unit_mask_host(T.SEED, (4, 100, 24), keep)
        assert set(np.unique(m)) == {0.0, np.float32(1.0 / keep)}
        assert abs((m > 0).mean() - keep) < 0.03


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("variant", ["plain", "g2", "den_g1", "leaky", "post", "drop_den"])
def test_closed_form_equals_float64_autograd(per_sample, variant):
    """oracle/norm_unit.unit against autograd through tf_ops.batch_norm / instance_norm with the TRUE statistics as the given ones."""
    rng = np.random.default_rng(5)
    n, hw, c = 3, 10, 8
    g = {"plain": 0, "g2": 2, "den_g1": 1, "leaky": 2, "post": 1, "drop_den": 0}[variant]
    den = variant in ("den_g1", "post", "drop_den")
    leaky = {"leaky": 2, "post": 3}.get(variant, 0)
    eps = 1e-6 if per_sample else 1e-3
    y = rng.standard_normal((n, hw, c)) * 2 + 0.5
    gamma, beta = rng.random(c) - 0.3, rng.standard_normal(c) * 0.3
    dz = rng.standard_normal((n, hw, c))
    dn = rng.random((n, c)) + 0.5 if den else None
    guide = rng.random((n, hw, g)) if g else None
    gw = rng.standard_normal((1, g, c)) * 0.5 if g else None
    gb = None
    if g or variant == "drop_den":
        gb = rng.standard_normal((1, c)) * 0.2
        if leaky == 3:
            ap = rng.integers(0, 2, (1, c)).astype(np.float64)
            gb = np.stack([gb, ap, 1 - ap, rng.standard_normal((1, c)) * 0.2], 1)
    mask = T.unit_mask_host(7, (n, hw, c), 0.5).astype(np.float64) if variant == "drop_den" else None
    ax = (1,) if per_sample else (0, 1)
    ns = n if per_sample else 1
    mean = y.mean(ax).reshape(ns, c)
    rstd = 1.0 / np.sqrt(y.var(ax).reshape(ns, c) + eps)
    scale = gamma[None] * rstd
    shift = beta[None] - mean * scale
    ref = norm_unit.unit(y, dz, mean, rstd, scale, shift, per_sample, den=dn, guide=guide, gw=gw, gb=gb, mask=mask, leaky=leaky,
                         alpha=0.3)
    t64 = lambda v: None if v is None else torch.tensor(v, dtype=torch.float64, requires_grad=True)
    ty, tg, tb, tden, tgw, tgb = t64(y.reshape(n, hw, 1, c)), t64(gamma), t64(beta), t64(dn), t64(gw), t64(gb)
    if per_sample:
        t = tf_ops.instance_norm(ty, tg, tb, eps=eps)
    else:
        t, _, _ = tf_ops.batch_norm(ty, tg, tb, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64), True, eps=eps)
    u = t.reshape(n, hw, c)
    if mask is not None:
        u = u * torch.tensor(mask)
    if den:
        u = u * tden[:, None, :]
    if gb is not None:
        bias = tgb[:, 0] if leaky == 3 else tgb
        s = bias[:, None, :] + (torch.tensor(guide) @ tgw[0] if g else 0.0)
        if leaky == 3:
            u = u + torch.where(s > 0, tgb[:, 1][:, None, :], tgb[:, 2][:, None, :]).detach() * s + tgb[:, 3][:, None, :]
        elif leaky:
            u = u + torch.nn.functional.leaky_relu(s, 0.3)
        else:
            u = u + s
    z = torch.relu(u)
    z.backward(torch.tensor(dz))
    close = lambda got, want: np.allclose(got, want.numpy() if hasattr(want, "numpy") else want, rtol=1e-9, atol=1e-11)
    assert close(ref["z"], z.detach())
    assert close(ref["dy"], ty.grad.reshape(n, hw, c)) and close(ref["dgamma"], tg.grad) and close(ref["dbeta"], tb.grad)
    if den:
        assert close(ref["dden"], tden.grad)
    if g:
        assert close(ref["dgw"], tgw.grad)
    if gb is not None:
        want = tgb.grad.numpy().copy()
        assert close(ref["dgb"], want)
