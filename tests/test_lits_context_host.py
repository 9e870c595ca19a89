"""CPU: the context guide of the guided LiTS pipeline -- the per-slice histogram features (extract.py:237-375), the flags,
the guide coin it shares with the spatial guide, the --hist_noise build-up and the offline slab rows.

`hist_rows_numpy` restates both feature modes with numpy / scipy and is pinned here on the reference's own
`dump_hist_feature` / `dump_hist_feature_v2` (tests/golden/ref_hist_feature.npz, make_hist_fixtures.py); the host tables of
`unetk_slice_hist` (ops.hist_bin_table) are held to the same rows through an integer-count restatement of the kernel.
tests/test_gpu_lits_context.py holds the kernels against these restatements."""
import argparse
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

from boxsegliver_amd.data import lits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hist_feature.npz")
XRNG = (-200, 250)


def _density(values, bins, xrng):
    with np.errstate(invalid="ignore"):
        h, _ = np.histogram(values, bins=bins, range=xrng, density=True)
    return np.nan_to_num(h.astype(np.float32))


def hist_rows_numpy(vol, lab, mode, bins=100, xrng=XRNG):
    """float32 [D, 2 bins]: the liver (lab >= 1) density of each slice, then its tumour density -- mode "train": the
    slice's own lab == 2 pixels; mode "eval": for every 18-connected tumour whose z-extent [z0, z1) covers the slice, the
    tumour's pixels on its middle slice (z1 - z0 - 1) // 2 + z0."""
    d = vol.shape[0]
    out = np.empty((d, 2 * bins), np.float32)
    if mode == "eval":
        comp, _ = ndi.label(lab == 2, ndi.generate_binary_structure(3, 2))
        spans = [(s[0].start, s[0].stop) for s in ndi.find_objects(comp)]
    for k in range(d):
        out[k, :bins] = _density(vol[k][lab[k] >= 1], bins, xrng)
        if mode == "train":
            t = vol[k][lab[k] == 2]
        else:
            parts = [vol[(z1 - z0 - 1) // 2 + z0][comp[(z1 - z0 - 1) // 2 + z0] == c + 1]
                     for c, (z0, z1) in enumerate(spans) if z0 <= k < z1]
            t = np.concatenate(parts) if parts else np.zeros(0, vol.dtype)
        out[k, bins:] = _density(t, bins, xrng)
    return out


def hist_rows_counts(vol, lab, mode, bins=100, xrng=XRNG):
    """The kernel's arithmetic on the host: integer counts through ops.hist_bin_table, the eval half as a difference array
    over z per component, then (count / db) / total in float64 rounded to float32."""
    from boxsegliver_amd import ops
    lut, lo, db = ops.hist_bin_table(bins, xrng)
    v = vol.astype(np.int64) - lo
    b = np.where((v >= 0) & (v < len(lut)), lut[np.clip(v, 0, len(lut) - 1)], -1)
    d = vol.shape[0]
    counts = np.zeros((d, 2, bins), np.int64)
    for k in range(d):
        counts[k, 0] = np.bincount(b[k][(lab[k] >= 1) & (b[k] >= 0)], minlength=bins)
        if mode == "train":
            counts[k, 1] = np.bincount(b[k][(lab[k] == 2) & (b[k] >= 0)], minlength=bins)
    if mode == "eval":
        comp, _ = ndi.label(lab == 2, ndi.generate_binary_structure(3, 2))
        diff = np.zeros((d + 1, bins), np.int64)
        for c, s in enumerate(ndi.find_objects(comp)):
            z0, z1 = s[0].start, s[0].stop
            m = (z1 - z0 - 1) // 2 + z0
            sel = (comp[m] == c + 1) & (b[m] >= 0)
            h = np.bincount(b[m][sel], minlength=bins)
            diff[z0] += h
            diff[z1] -= h
        counts[:, 1] = np.cumsum(diff, axis=0)[:d]
    total = counts.sum(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        dens = (counts / db) / total
    return np.where(total > 0, dens, 0.).astype(np.float32).reshape(d, 2 * bins)


def _fixture():
    z = np.load(GOLDEN)
    n = len([k for k in z.files if k.startswith("vol_")])
    assert n >= 4
    return [(z["vol_%d" % i], z["lab_%d" % i], z["train_%d" % i], z["eval_%d" % i]) for i in range(n)]


def test_restatement_reproduces_the_reference_features_bit_for_bit():
    for vol, lab, train, ev in _fixture():
        assert train.dtype == ev.dtype == np.float32 and train.shape == (vol.shape[0], 200)
        np.testing.assert_array_equal(hist_rows_numpy(vol, lab, "train"), train)
        np.testing.assert_array_equal(hist_rows_numpy(vol, lab, "eval"), ev)


def test_kernel_arithmetic_reproduces_the_reference_features_bit_for_bit():
    for vol, lab, train, ev in _fixture():
        np.testing.assert_array_equal(hist_rows_counts(vol, lab, "train"), train)
        np.testing.assert_array_equal(hist_rows_counts(vol, lab, "eval"), ev)


def test_fixture_covers_the_corner_cases():
    cases = _fixture()
    vols = np.concatenate([c[0].ravel() for c in cases])
    edges = np.linspace(-200, 250, 101)
    assert np.any(vols < -200) and np.any(vols > 250) and np.any(vols == 250) and np.any(vols == -200)
    assert np.isin(edges[2:-1:2].astype(np.int16), vols).all()
    for vol, lab, train, ev in cases[:3]:
        assert np.all(train[0] == 0) and np.all(ev[0] == 0)                              # no liver
        assert np.any((train[:, :100].sum(1) > 0) & (train[:, 100:].sum(1) == 0))        # liver, no tumour
    s18, s6 = ndi.generate_binary_structure(3, 2), ndi.generate_binary_structure(3, 1)
    lab1, lab2 = cases[1][1] == 2, cases[2][1] == 2
    assert ndi.label(lab1, s18)[1] < ndi.label(lab1, s6)[1]                               # edge contacts join under 18
    assert ndi.label(lab2, s18)[1] == ndi.label(lab2, ndi.generate_binary_structure(3, 3))[1] + 2   # corners do not
    assert np.any(cases[0][3] != cases[0][2])                                            # eval differs from train


def test_bin_table_follows_numpys_edges():
    from boxsegliver_amd import ops
    lut, lo, db = ops.hist_bin_table(100, XRNG)
    assert lo == -200 and len(lut) == 451 and np.all(db == 4.5) and db.dtype == np.float64
    assert lut[0] == 0 and lut[-1] == 99 and lut[-2] == 99 and np.all(np.diff(lut) >= 0)
    v = np.arange(-200, 251)
    ref = np.array([np.argmax(np.histogram([x], bins=100, range=XRNG)[0]) for x in v])
    np.testing.assert_array_equal(lut, ref)
    lut2, lo2, _ = ops.hist_bin_table(7, (-3.5, 10.2))                                    # non-integer range
    assert lo2 == -3 and len(lut2) == 14 and lut2.min() >= 0 and lut2.max() == 6


# ------------------------------------------------------------------------------------------------- flags
def test_context_list_parsing():
    assert lits.parse_context_list(["hist", "200"]) == [("hist", 200)]
    assert lits.parse_context_list(["hist", "100", "hist", "200"]) == [("hist", 100), ("hist", 200)]
    with pytest.raises(ValueError, match="paired"):
        lits.parse_context_list(["hist", "200", "hist"])
    with pytest.raises(ValueError, match="glcm.*not supported"):
        lits.parse_context_list(["glcm", "96"])
    with pytest.raises(ValueError, match="--context_list"):
        lits.parse_context_list(None)


def test_context_rows_load_scale_and_errors(tmp_path):
    cases = [{"PID": 3, "size": [4, 8, 8]}, {"PID": 12, "size": [2, 8, 8]}]
    d = tmp_path / "feat" / "hist" / "train"
    d.mkdir(parents=True)
    rng = np.random.default_rng(0)
    a, b = rng.random((4, 200)).astype(np.float32), rng.random((2, 200)).astype(np.float32)
    np.save(d / "003.npy", a)
    np.save(d / "012.npy", b)
    rows = lits.load_context_rows(tmp_path, cases, {3: 2, 12: 0}, 6, [("hist", 200)], "train", 20.)
    assert rows.dtype == np.float32 and rows.shape == (6, 200)
    ref_a = a.copy()
    ref_a *= 20.                                                              # feature_ops.hist_preprocess
    np.testing.assert_array_equal(rows[2:6], ref_a)
    np.testing.assert_array_equal(rows[0:2], b * np.float32(20.))
    with pytest.raises(ValueError, match="length mismatch"):
        lits.load_context_rows(tmp_path, cases, {3: 2, 12: 0}, 6, [("hist", 100)], "train", 20.)
    with pytest.raises(FileNotFoundError, match="eval.*003.npy.*extract hist"):
        lits.load_context_rows(tmp_path, cases, {3: 2, 12: 0}, 6, [("hist", 200)], "eval", 20.)


# ------------------------------------------------------------------------------------------------- coin and noise
CFG = argparse.Namespace(im_height=48, im_width=48, im_channel=3)


def _sampler(context, guide=True, seed=5):
    from test_lits_guide_host import _case
    cases = [_case(i) for i in range(3)]
    g = lits.GuidePolicy(spatial_random=0.5) if guide else None
    return lits.TrainSampler(cases, 16, CFG, liver_percent=0.66, tumor_percent=0.5, random_scale=(1.0, 1.4),
                             random_window_level=True, random_flip=3, seed=seed, guide=g, context=context)


def test_spatial_guide_and_context_share_one_coin():
    """With both guides the coin is drawn once (guide_coin) and handed to guide_objects: the objects are those of a
    spatial-only sampler, whose guide_objects draws the same coin itself; the batches are unchanged."""
    both, alone = _sampler(True), _sampler(False)
    for _ in range(6):
        b1, b2 = both.draw(), alone.draw()
        assert all(np.array_equal(b1[k], b2[k]) for k in ("case", "z", "box", "flips"))
        coin = both.guide_coin(0.5)
        p1, o1 = both.guide_objects(b1, coin)
        p2, o2 = alone.guide_objects(b2)
        np.testing.assert_array_equal(p1, p2)
        np.testing.assert_array_equal(o1, o2)
        # a sample whose coin failed has no guide objects (and gets a zero context row)
        assert np.all(np.diff(p1)[~coin] == 0)
    # the context alone still draws its coin from the guide generator, not from the batch stream
    ctx, plain = _sampler(True, guide=False), _sampler(False, guide=False)
    for _ in range(3):
        b1, b2 = ctx.draw(), plain.draw()
        assert all(np.array_equal(b1[k], b2[k]) for k in ("case", "z", "box", "flips"))
        c = ctx.guide_coin(0.5)
        assert c.dtype == bool and c.shape == (16,)


def context_numpy(table, idx, take, noise=None):
    """unetk_lits_context restated: samples in order, in-place float32 += float64 noise (numpy's rounding), zeros where
    the coin failed or the slice is padding.  Returns (out, table after the batch)."""
    table = table.copy()
    out = np.zeros((len(idx), table.shape[1]), np.float32)
    for s, (i, t) in enumerate(zip(idx, take)):
        if t and 0 <= i < len(table):
            if noise is not None:
                feat = table[i]                       # a view into the cached table, as the reference's
                feat += noise[s]
            out[s] = table[i]
    return out, table


def test_noise_builds_up_in_the_table():
    rng = np.random.default_rng(1)
    table = rng.random((5, 6)).astype(np.float32)
    idx = np.array([2, 4, 2, -1, 0])
    take = np.array([1, 1, 1, 1, 0])
    noise = rng.normal(0., 1., (5, 6)) * 0.002
    out, after = context_numpy(table, idx, take, noise)
    first = (table[2].astype(np.float64) + noise[0]).astype(np.float32)
    second = (first.astype(np.float64) + noise[2]).astype(np.float32)
    np.testing.assert_array_equal(out[0], first)
    np.testing.assert_array_equal(out[2], second)                          # the duplicate sees the first update
    np.testing.assert_array_equal(after[2], second)
    assert np.all(out[3] == 0) and np.all(out[4] == 0)                     # padding, failed coin
    np.testing.assert_array_equal(after[0], table[0])                      # a failed coin adds no noise
    np.testing.assert_array_equal(after[[1, 3]], table[[1, 3]])
    # the next batch starts from the updated rows
    out2, _ = context_numpy(after, np.array([2]), np.array([1]), noise[:1])
    np.testing.assert_array_equal(out2[0], (second.astype(np.float64) + noise[0]).astype(np.float32))


# ------------------------------------------------------------------------------------------------- offline slabs
def _reference_slab_rows(bbox, lhc, rhc, n_vol, batch_size):
    """input_pipeline_g.py:955-969 literally: `for idx in range(lhc, volume.shape[-1] - rhc, batch_size): sid = bbox[2] +
    idx - lhc`, context_val[sid:sid + batch_size]."""
    return [(bbox[2] + idx - lhc, bbox[2] + idx - lhc + batch_size) for idx in range(lhc, n_vol - rhc, batch_size)]


@pytest.mark.parametrize("z1,z2,depth,bs,c", [(3, 10, 14, 4, 3), (0, 14, 14, 4, 3), (5, 14, 14, 8, 1), (2, 3, 6, 4, 5)])
def test_offline_slab_rows_follow_the_reference(z1, z2, depth, bs, c):
    lhc, rhc = (c - 1) // 2, c - 1 - (c - 1) // 2
    pads = (bs - ((z2 - z1) % bs)) % bs
    n = z2 - z1 + pads
    ours = lits.slab_context_rows(z1, n, bs)
    assert ours == _reference_slab_rows([0, 0, z1], lhc, rhc, n + lhc + rhc, bs)
    # the rows past the liver box read the next real slices, then the pad rows appended at the end; never out of range
    assert ours[-1][1] == z2 + pads <= depth + pads


def test_eval_context_pads_rows_at_the_end(tmp_path):
    d = tmp_path / "feat" / "hist" / "eval"
    d.mkdir(parents=True)
    rows = np.arange(5 * 200, dtype=np.float32).reshape(5, 200)
    np.save(d / "007.npy", rows)
    torch = pytest.importorskip("torch")
    ec = lits.EvalContext(tmp_path, [("hist", 200)], 2.0, device=torch.device("cpu"))
    t = ec.case({"PID": 7, "size": [5, 8, 8]}, 3)
    assert tuple(t.shape) == (8, 200) and t.dtype == torch.float32
    np.testing.assert_array_equal(t[:5].numpy(), rows * np.float32(2.0))
    assert bool((t[5:] == 0).all())


def test_noise_draws_leave_the_guide_stream_alone():
    """The --hist_noise normals come from a generator of their own: the coins and guide objects of later batches are those
    of a run without noise."""
    a, b = _sampler(True), _sampler(True)
    for _ in range(4):
        ba, bb = a.draw(), b.draw()
        ca, cb = a.guide_coin(0.5), b.guide_coin(0.5)
        np.testing.assert_array_equal(ca, cb)
        pa, oa = a.guide_objects(ba, ca)
        pb, ob = b.guide_objects(bb, cb)
        np.testing.assert_array_equal(oa, ob)
        a.noise_rng.normal(0., 1., (16, 200))                             # only `a` draws noise
