"""tests/small_ops_cases.py without a GPU: the float64 restatements against independent references, the exactness conditions of
every exact-tier row, and the coverage of the table (every path of DESIGN.md 6.6 has a row, every grid cap one row exactly at it
and one over it with a ragged second pass)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ops_cases as T
from oracle import interunet2d, tf_ops

SMALL = [r for r in T.ROWS if "cap" not in r.id]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _ids(fam, pred=lambda r: True):
    return [r.id for r in SMALL if r.fam == fam and pred(r)]


# ------------------------------------------------------------------ restatements against independent references
def _tie_free(shape, seed):
    """Distinct values: a permutation of 0 .. n - 1, centred."""
    n = int(np.prod(shape))
    return (np.random.default_rng(seed).permutation(n).astype(np.float64) - n // 2).reshape(shape)


@pytest.mark.parametrize("rid", _ids("mp2"))
def test_maxpool2_restatement_against_autograd(rid):
    p = T.BY_ID[rid].p
    x = _t(_tie_free((p["n"], p["h"], p["w"], p["c"]), 1)).requires_grad_()
    y = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert np.array_equal(T.maxpool2_fwd(x.detach().numpy()), y.detach().numpy())
    if p["h"] % 2 == 0 and p["w"] % 2 == 0:
        dp = np.random.default_rng(2).integers(-2, 3, size=tuple(y.shape)).astype(np.float64)
        add = np.random.default_rng(3).integers(-2, 3, size=tuple(x.shape)).astype(np.float64)
        y.backward(_t(dp))
        assert np.array_equal(T.maxpool2_bwd(x.detach().numpy(), dp), x.grad.numpy())
        assert np.array_equal(T.maxpool2_bwd(x.detach().numpy(), dp, add), x.grad.numpy() + add)


@pytest.mark.parametrize("rid", _ids("mp2", lambda r: r.p["h"] % 2 == 0 and r.p["w"] % 2 == 0))
@pytest.mark.parametrize("storage", [T.FP32S, T.BF16S])
def test_maxpool2_restatement_on_ties_against_a_window_loop(rid, storage):
    row = T.BY_ID[rid]
    a = T.make_inputs(row, "exact", storage)
    x, dp = a["x"], a["dp"]
    n, h, w, c = x.shape
    want_p, want_dx = np.zeros((n, h // 2, w // 2, c)), np.zeros_like(x)
    for i in range(n):
        for ho in range(h // 2):
            for wo in range(w // 2):
                for ch in range(c):
                    best, at = -np.inf, None
                    for dh in range(2):
                        for dw in range(2):
                            v = x[i, 2 * ho + dh, 2 * wo + dw, ch]
                            if v > best:                           # strictly greater: the first maximum keeps the gradient
                                best, at = v, (dh, dw)
                    want_p[i, ho, wo, ch] = best
                    want_dx[i, 2 * ho + at[0], 2 * wo + at[1], ch] = dp[i, ho, wo, ch]
    ref = T.reference(row, a, storage)
    assert np.array_equal(ref["p"], want_p)
    assert np.array_equal(ref["dx"], want_dx + (a["add"] if a["add"] is not None else 0.0))


@pytest.mark.parametrize("rid", [r.id for r in T.rows("mp2")])
@pytest.mark.parametrize("storage", [T.FP32S, T.BF16S])
def test_pool_rows_carry_the_edge_content(rid, storage):
    """Every max-pool row, the one-window row and the cap rows (their repeated block) included."""
    row = T.BY_ID[rid]
    a = T.make_inputs(row, "exact", storage)
    if "blk" in a:
        storage, a = T.BF16S, a["blk"]                                # the cap rows carry the rounded tie channel in both storages
    win = T.windows2(a["x"])
    chans = [c for c in range(win.shape[-1]) if not (storage == T.BF16S and c == 1)]
    wn = win[..., chans]
    mx = wn.max(axis=3, keepdims=True)
    assert ((wn == mx).sum(axis=3) == 4).any(), "no window of four equal values"
    first = np.argmax(wn, axis=3)
    single = (wn == mx).sum(axis=3) == 1
    for place in range(4):
        assert (single & (first == place)).any(), "no window with its only maximum at place %d" % place
    zero = (wn == 0).all(axis=3)
    sign = np.signbit(wn)
    assert (zero & sign[:, :, :, 0] & ~sign.all(axis=3)).any() and (zero & ~sign[:, :, :, 0] & sign.any(axis=3)).any(), \
        "no window mixing -0.0 and +0.0 in both orders"
    assert ((wn == 0) & ~zero[:, :, :, None] & (a["dp"][:, :, :, None, chans] != 0)).any(), "no zero pixel under a non-zero gradient"
    if storage == T.BF16S:
        raw = win[..., 1]
        assert np.array_equal(raw, T.round_bf16(raw)) and ((raw == raw.max(axis=3, keepdims=True)).sum(axis=3) > 1).any()
        assert (np.abs(raw - 64.0) <= 1.0).all()


@pytest.mark.parametrize("rid", _ids("mp1"))
def test_maxpool1d_restatement(rid):
    p = T.BY_ID[rid].p
    x = _t(_tie_free((p["b"], p["l"], p["c"]), 4)).requires_grad_()
    y = F.max_pool1d(x.permute(0, 2, 1), 2, ceil_mode=True).permute(0, 2, 1)
    assert np.array_equal(T.maxpool1d_fwd(x.detach().numpy()), y.detach().numpy())
    dy = np.random.default_rng(5).integers(-2, 3, size=tuple(y.shape)).astype(np.float64)
    y.backward(_t(dy))
    assert np.array_equal(T.maxpool1d_bwd(x.detach().numpy(), dy), x.grad.numpy())
    # ties: a hand-written window loop, the first maximum takes the gradient
    a = T.make_inputs(T.BY_ID[rid], "exact")
    xe, de = a["x"], a["dy"]
    want_y, want_dx = np.zeros_like(de), np.zeros_like(xe)
    for b in range(p["b"]):
        for lo in range((p["l"] + 1) // 2):
            for c in range(p["c"]):
                second = 2 * lo + 1 < p["l"] and xe[b, 2 * lo + 1, c] > xe[b, 2 * lo, c]
                want_y[b, lo, c] = xe[b, 2 * lo + 1, c] if second else xe[b, 2 * lo, c]
                want_dx[b, 2 * lo + (1 if second else 0), c] = de[b, lo, c]
    assert np.array_equal(T.maxpool1d_fwd(xe), want_y) and np.array_equal(T.maxpool1d_bwd(xe, de), want_dx)
    if p["l"] >= 7 and p["c"] >= 16:
        pair = xe[:, :p["l"] // 2 * 2].reshape(p["b"], -1, 2, p["c"])
        assert (pair[:, :, 0] == pair[:, :, 1]).any() and (pair[:, :, 0] > pair[:, :, 1]).any() and (pair[:, :, 0] < pair[:, :, 1]).any()


@pytest.mark.parametrize("rid,tier", [(r, t) for r in _ids("fc") for t in ("exact", "gauss") if t == "gauss" or T.exact_tier(T.BY_ID[r])])
def test_fc_restatement_against_autograd(rid, tier):
    row = T.BY_ID[rid]
    p = row.p
    a = T.make_inputs(row, tier)
    x, w = _t(a["x"]).requires_grad_(), _t(a["w"]).requires_grad_()
    b = _t(a["b"]).requires_grad_() if p["bias"] else None
    pre = x @ w + (b if b is not None else 0.0)
    y = pre if p["relu"] == 0 else (torch.relu(pre) if p["relu"] == 1 else torch.sigmoid(pre))
    if a["mask"] is not None:
        y = y * _t(a["mask"])
    y.backward(_t(a["dy"]))
    ref = T.reference(row, a)
    close = (lambda u, v: np.array_equal(u, v)) if tier == "exact" else (lambda u, v: np.allclose(u, v, rtol=1e-12, atol=1e-12))
    assert close(ref["y"], y.detach().numpy()) and close(ref["dw"], w.grad.numpy()) and close(ref["dx"], x.grad.numpy())
    if b is not None:
        assert close(ref["db"], b.grad.numpy())
    if a["mask"] is not None:
        share = (a["mask"] != 0).mean()
        assert set(np.unique(a["mask"])) <= {0.0, 1.0 / p["keep"]} and abs(share - p["keep"]) < 0.25


@pytest.mark.parametrize("rid", _ids("conv1d"))
@pytest.mark.parametrize("tier", ["exact", "gauss"])
def test_conv1d_restatement_against_autograd(rid, tier):
    row = T.BY_ID[rid]
    p = row.p
    a = T.make_inputs(row, tier)
    x, w = _t(a["x"]).requires_grad_(), _t(a["w"]).requires_grad_()
    b = _t(a["b"]).requires_grad_() if p["bias"] else None
    pre = F.conv1d(x.permute(0, 2, 1), w.permute(2, 1, 0), b, padding=p["k"] // 2).permute(0, 2, 1)
    y = torch.relu(pre) if p["relu"] else pre
    y.backward(_t(a["dy"]))
    ref = T.reference(row, a)
    close = (lambda u, v: np.array_equal(u, v)) if tier == "exact" else (lambda u, v: np.allclose(u, v, rtol=1e-12, atol=1e-12))
    assert close(ref["y"], y.detach().numpy()) and close(ref["dw"], w.grad.numpy()) and close(ref["dx"], x.grad.numpy())
    if b is not None:
        assert close(ref["db"], b.grad.numpy())


@pytest.mark.parametrize("rid", [r.id for r in SMALL if r.fam in ("fc", "conv1d") and r.p["relu"] == 1])
def test_relu_rows_have_zero_preactivations_that_a_ge_gate_would_pass(rid):
    row = T.BY_ID[rid]
    a = T.make_inputs(row, "exact")
    ref = T.reference(row, a)
    wrong = T.fc(a, 1, ge=True) if row.fam == "fc" else T.conv1d(a, row.p["k"], 1, ge=True)
    m = a.get("mask")
    live = (ref["pre"] == 0) & (a["dy"] != 0) & ((m != 0) if m is not None else True)
    assert live.any(), "no pre-activation at exactly 0 under a non-zero gradient"
    assert (ref["dpre"][ref["pre"] == 0] == 0).all()
    assert (ref["pre"] < 0).any() and (ref["pre"] > 0).any() or row.p.get("n") == 1
    assert not np.array_equal(wrong["dpre"], ref["dpre"])
    outs = [k for k in ("db", "dw", "dx") if row.p.get(k, True)]
    assert any(not np.array_equal(wrong[k], ref[k]) for k in outs), "a >= 0 gate gives the same sums: the row cannot tell"


@pytest.mark.parametrize("rid", _ids("sobel"))
def test_sobel_restatement_against_the_oracle(rid):
    row = T.BY_ID[rid]
    for tier in ("exact", "gauss"):
        a = T.make_inputs(row, tier)
        want = interunet2d.sobel_concat(_t(a["x"]), row.p["ch"]).numpy()
        got = T.sobel_concat(a["x"], row.p["ch"])
        assert np.array_equal(got, want) if tier == "exact" else np.allclose(got, want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("rid", _ids("ig") + _ids("avg"))
def test_image_gradients_and_avgpool_restatements_against_the_oracle(rid):
    row = T.BY_ID[rid]
    for tier in ("exact", "gauss"):
        x = T.make_inputs(row, tier)["x"]
        if row.fam == "ig":
            want = torch.cat((_t(x),) + tf_ops.image_gradients(_t(x)), dim=-1).numpy()
            assert np.array_equal(T.image_gradients(x), want)
        else:
            want = tf_ops.avg_pool2x2_same(_t(x)).numpy()
            assert np.allclose(T.avgpool2_fwd(x), want, rtol=1e-15, atol=1e-15)


def test_flip_moments_and_spatial_mean_restatements():
    rng = np.random.default_rng(6)
    x, o = rng.standard_normal((2, 3, 5, 2)), rng.standard_normal((2, 3, 5, 2))
    for fh in (0, 1):
        for fw in (0, 1):
            want = 0.5 * np.flip(x, axis=tuple(ax for ax, f in ((1, fh), (2, fw)) if f)) if (fh or fw) else 0.5 * x
            assert np.array_equal(T.flip_axpy(x, o, fh, fw, 0.5, 0), want)
            assert np.array_equal(T.flip_axpy(x, o, fh, fw, 0.5, 1), want + o)
    g = rng.standard_normal((3, 7, 2))
    per = T.guide_moments(g, 1)
    assert per.shape == (3, 6)
    for n in range(3):
        assert np.allclose(per[n, :2], g[n].mean(0)) and np.allclose(per[n, 2 + 1 * 2 + 0], (g[n][:, 1] * g[n][:, 0]).mean())
    allg = T.guide_moments(g, 0)
    assert allg.shape == (1, 6) and np.allclose(allg[0, 2 + 0 * 2 + 1], (g[..., 0] * g[..., 1]).mean())
    xs = _t(rng.standard_normal((3, 5, 4))).requires_grad_()
    dy = rng.standard_normal((3, 4))
    xs.mean(dim=1).backward(_t(dy))
    assert np.allclose(T.spatial_mean_fwd(xs.detach().numpy()), xs.detach().mean(dim=1).numpy(), rtol=1e-15)
    assert np.allclose(T.spatial_mean_bwd(dy, 5), xs.grad.numpy(), rtol=1e-15)


def test_spatial_mean_bound_is_four_times_the_measured_error():
    """The bound tier's bound for spatial_mean_fwd: the float32 restatement of the kernel's summation order against float64 on the
    rows' own inputs, times four."""
    worst = 0.0
    for row in T.rows("smean"):
        x = T.make_inputs(row, "gauss")["x"]
        ref = T.spatial_mean_fwd(x)
        e = np.abs(T.spatial_mean_fwd_f32(x).astype(np.float64) - ref).max() / np.abs(ref).max()
        print(row.id, e)
        worst = max(worst, e)
    assert 0.5 * T.SPATIAL_MEAN_MEASURED < worst <= T.SPATIAL_MEAN_MEASURED and T.SPATIAL_MEAN_REL == 4 * T.SPATIAL_MEAN_MEASURED
    # the two roundings of the backward are exact where HW is a power of two
    for row in T.rows("smean"):
        dy = T.make_inputs(row, "exact")["dy"]
        hw = row.p["hw"]
        if hw & (hw - 1) == 0:
            assert np.array_equal(T.spatial_mean_bwd_f32(dy, hw), T.spatial_mean_bwd(dy, hw))


def test_boundary_rows_and_the_ring_free_closed_form():
    for row in T.rows("boundary"):
        lab = T.boundary_labels(row)
        assert lab.shape == (row.p["n"], row.p["h"], row.p["w"]) and lab.dtype == np.int32
    single = T.boundary_labels(T.BY_ID["bw_single_between"])
    assert len(np.unique(single[1])) == 1 and len(np.unique(single[0])) > 1 and len(np.unique(single[2])) > 1
    stripes = T.boundary_labels(T.BY_ID["bw_stripes"])
    changes = (stripes[:, :, 1:] != stripes[:, :, :-1]).any(axis=(0, 1))
    assert 0 < changes.sum() < 0.25 * changes.size                  # most columns hold no ring pixel
    b = T.boundary_labels(T.BY_ID["bw_borders"])
    for edge in (b[:, 0, :], b[:, -1, :], b[:, :, 0], b[:, :, -1]):
        assert all(len(np.unique(e)) > 1 for e in edge)
    # ring-free: the oracle's map over its own scale is the closed form
    row = T.BY_ID["bw_ringfree"]
    w = T.boundary_weights(T.boundary_labels(row))
    v = T.boundary_ringfree_unscaled(row.p["h"], row.p["w"])
    for n in range(row.p["n"]):
        np.testing.assert_allclose(w[n] / w[n, 0, 0], v / v[0, 0], rtol=T.BOUNDARY_RTOL)
    assert T.boundary_ws_bytes(2, 3, 5) == (30 + 6 + 2 + 64) * 4


# ------------------------------------------------------------------ exactness conditions
def _multiple(a, unit):
    q = np.asarray(a, np.float64) / unit
    return bool(np.all(q == np.round(q)))


@pytest.mark.parametrize("rid", [r.id for r in T.ROWS if T.exact_tier(r)])
def test_exact_tier_is_exact(rid):
    """All summands multiples of one power of two, the sum of their magnitudes below 2^24 units, every stored value representable."""
    row = T.BY_ID[rid]
    for storage in T.storages(row):
        a = T.make_inputs(row, "exact", storage)
        for name, unit, mag, ints, units in T.exact_sums(row, a):
            assert np.log2(unit) == int(np.log2(unit))
            assert all(_multiple(i, 1.0) for i in ints) and all(_multiple(u, unit) for u in units), (rid, name)
            assert len(units) <= 1 or not ints or name == "pre", (rid, name)       # pre: x * w and the bias, both unit multiples
            assert mag < 2 ** 24, (rid, name, mag)
        for key, v in a.items():
            if v is not None and key not in ("labels", "blk"):
                assert np.array_equal(T.store(v, storage), v), (rid, key)
        ref = T.reference(row, a, storage)
        for key, v in ref.items():
            if (row.fam, key) in (("smean", "y"), ("smean", "dx"), ("moments", "out")):
                continue                                                            # one division: compared after ONE rounding
            assert np.array_equal(T.store(v, storage), v), (rid, key)


def test_exact_tier_parameters():
    for row in T.ROWS:
        if row.fam == "flip":
            assert row.p["scale"] in (0.5, 1.0, 2.0)
        if row.fam == "fc":
            assert row.p["keep"] in (None, 0.5, 0.25)
            assert row.p["relu"] < 2 or row.p["keep"] is None           # the sigmoid with a mask is refused (include/unetk.h)


# ------------------------------------------------------------------ coverage of the table
@pytest.mark.parametrize("path", T.PATHS, ids=["%s: %s" % (p[2], p[0]) for p in T.PATHS])
def test_every_path_has_a_row(path):
    assert T.rows_of(path), path[0]


@pytest.mark.parametrize("cap", T.CAPS, ids=[c[0] for c in T.CAPS])
def test_every_cap_has_a_row_at_it_and_a_ragged_row_over_it(cap):
    name, fam, threads, limit = cap
    at, over = T.cap_rows(cap)
    assert len(at) == 1 and len(over) == 1, (name, at, over)
    t = threads(T.BY_ID[over[0]].p)
    assert limit < t < 2 * limit and (t - limit) % limit != 0, (name, t)          # a second pass that not every thread takes
    assert T.BY_ID[at[0]].fam == T.BY_ID[over[0]].fam == fam


@pytest.mark.parametrize("rid", [r.id for r in T.ROWS])
def test_no_expected_output_is_identically_zero(rid):
    """A row whose reference is all zeros compares nothing but the write coverage."""
    row = T.BY_ID[rid]
    for tier in ("exact", "gauss"):
        if tier == "exact" and not T.exact_tier(row) and row.fam != "boundary":
            continue
        a = T.make_inputs(row, tier)
        if "blk" in a:                                                 # the repeated block stands for the row
            a, row = dict(a["blk"], add=None), row._replace(p=dict(row.p, h=74, w=82))
        for key, v in T.reference(row, a).items():
            if key in ("pre", "dpre") or not row.p.get(key, True):
                continue
            assert np.any(v != 0), (rid, tier, key)
            if row.fam in ("fc", "conv1d") and key != "db" and v.size >= 64:       # ReLU and keep 1/4 leave an eighth alive
                assert np.mean(v != 0) > 0.1, (rid, tier, key, np.mean(v != 0))


@pytest.mark.parametrize("cap", T.CAPS, ids=[c[0] for c in T.CAPS])
def test_cap_rows_are_live_in_both_passes(cap):
    """The over-cap row's expected outputs are non-zero below the cap and in the ragged second pass, so that a second pass that
    reads the wrong place is seen, not only one that writes nothing."""
    name, fam, threads, limit = cap
    row = T.BY_ID[T.cap_rows(cap)[1][0]]
    per = {"mp2": 4}.get(fam, 1)                                      # elements per thread
    key = {"mp2": "dx", "avg": "p", "ig": "out", "sobel": "out", "flip": "out", "smean": "dx", "mp1": "dx", "boundary": "wmap"}.get(fam)
    if fam == "conv1d":
        key = "dx" if "bwd_x" in name else ("dw" if "bwd_w" in name else "y")
    ref = T.reference(row, T.make_inputs(row, "exact"))[key]
    if fam == "boundary":
        flat = ref[0].reshape(-1)
    elif fam == "mp2":
        flat = T.maxpool2_fwd(np.abs(ref)).reshape(-1)               # one value per window and channel, in thread order
    else:
        flat = ref.reshape(-1)
    share = lambda v: np.mean(v != 0)
    per = flat.size // (threads(row.p) if fam != "boundary" else flat.size)
    first, second = flat[:limit * per], flat[limit * per:]
    assert second.size > 0 and share(first) > 0.2 and share(second) > 0.2, (name, share(first), share(second))


def test_row_ids_are_unique_and_small_rows_are_small():
    assert len({r.id for r in T.ROWS}) == len(T.ROWS)
    for r in SMALL:
        a = T.make_inputs(r, "gauss")
        assert sum(v.size for v in a.values() if v is not None and not isinstance(v, dict)) < 1 << 20, r.id
