"""Host side of the `glcm` context guide (no GPU): a numpy restatement of the co-occurrence counting rule, of the reference's
property formulas (utils/array_kits.py:1140-1232) and of its two dump loops (DataLoader/Liver/extract.py:377-661) against
the rows recorded from the reference itself (tests/golden/ref_glcm_feature.npz, made by tests/golden/make_glcm_fixtures.py);
the offsets table; the --glcm gate of the context list and its refusals; the preprocessing of the loaded rows; the noise
scale vector.  tests/test_gpu_glcm.py imports the restatement as the reference of the device op."""
import argparse
import functools
import json
import math
import os
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_glcm_feature.npz")
OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, 2), (1, 1), (2, 0), (1, -1), (0, 3), (2, 2), (3, 0), (2, -2))
PROPS = ("contrast", "dissimilarity", "homogeneity", "energy", "entropy", "correlation", "cluster_shade", "cluster_prominence")
SCALE = np.array([1 / 4096., 1 / 64., 2., 2., 1 / 8., 1., 1 / 64. ** 3, 1 / 64. ** 4])


# ------------------------------------------------------------------------------------------------- the restatement
def glcm_counts_numpy(patch, offsets=OFFSETS):
    """uint32 [K, 256, 256]: S = C + C^T, C[a][b] = the pixels (r, c) with value a whose partner (r + dr, c + dc) lies inside
    the patch and has value b (sliced np.add.at)."""
    h, w = patch.shape
    out = np.zeros((len(offsets), 256, 256), dtype=np.uint32)
    for k, (dr, dc) in enumerate(offsets):
        r0, r1, c0, c1 = max(0, -dr), min(h, h - dr), max(0, -dc), min(w, w - dc)
        if r1 <= r0 or c1 <= c0:
            continue
        c = np.zeros((256, 256), dtype=np.uint32)
        np.add.at(c, (patch[r0:r1, c0:c1].reshape(-1), patch[r0 + dr:r1 + dr, c0 + dc:c1 + dc].reshape(-1)), 1)
        out[k] = c + c.T
    return out


def glcm_counts_brute(patch, offsets=OFFSETS):
    """The same by the plain double loop over the pixels: the definition."""
    h, w = patch.shape
    out = np.zeros((len(offsets), 256, 256), dtype=np.uint32)
    for k, (dr, dc) in enumerate(offsets):
        for r in range(h):
            for c in range(w):
                if 0 <= r + dr < h and 0 <= c + dc < w:
                    a, b = int(patch[r, c]), int(patch[r + dr, c + dc])
                    out[k, a, b] += 1
                    out[k, b, a] += 1
    return out


def glcm_props_numpy(s, norm_levels=True):
    """(values float64 [8], S_f float64 [8]) of one symmetric count matrix: the reference's greycoprops formulas on
    P = S / sum(S) (a zero sum taken as 1), and per property the sum of the absolute values of its terms (1 for correlation),
    both with glcm_features' scaling when norm_levels.  Only the non-zero entries are visited: zero entries add exactly 0."""
    i, j = np.nonzero(s)
    total = float(s.sum(dtype=np.uint64)) or 1.0
    p = s[i, j].astype(np.float64) / total
    i, j = i.astype(np.float64), j.astype(np.float64)
    d = i - j
    terms = [p * d ** 2, p * np.abs(d), p / (1. + d ** 2), p ** 2, p * np.log(p + 1e-16)]
    mi, mj = np.sum(i * p), np.sum(j * p)
    di, dj = i - mi, j - mj
    si, sj = np.sqrt(np.sum(p * di ** 2)), np.sqrt(np.sum(p * dj ** 2))
    cov = np.sum(p * (di * dj))
    corr = 1.0 if (si < 1e-15 or sj < 1e-15) else cov / (si * sj)
    shade, prom = p * (di + dj) ** 3, p * (di + dj) ** 4
    vals = np.array([terms[0].sum(), terms[1].sum(), terms[2].sum(), np.sqrt(terms[3].sum()), -terms[4].sum(), corr,
                     shade.sum(), prom.sum()])
    mags = np.array([np.abs(t).sum() for t in terms] + [1.0, np.abs(shade).sum(), np.abs(prom).sum()])
    if norm_levels:
        vals, mags = vals * SCALE, mags * SCALE                 # powers of two: the same bits as the reference's divisions
    return vals, mags


def glcm_features_numpy(patch, offsets=OFFSETS, norm_levels=True, counts=None):
    """(float64 [8 K], S_f [8 K]) of a patch in the reference's layout: column = property * K + offset index."""
    counts = glcm_counts_numpy(patch, offsets) if counts is None else counts
    both = [glcm_props_numpy(s, norm_levels) for s in counts]
    return (np.stack([v for v, _ in both], axis=1).reshape(-1), np.stack([m for _, m in both], axis=1).reshape(-1))


def _smooth(image, loop=0):
    if loop:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            image = ndi.zoom(image, (1. + loop * .1,) * 2, order=1)
    return ndi.gaussian_filter(image, 0.5)


def to_uint8(volume):
    return ((np.clip(volume, -250, 300) + 250) * (255. / 550)).astype(np.uint8)


def glcm_rows_numpy(volume, case, mode, features=glcm_features_numpy):
    """(rows float32 [depth, 96], S_f float64 [depth, 96]) as the reference's dump loops make them (filter_size 20,
    average_num 3); S_f of a row = the mean of its patches' S_f (eval: accumulated and divided like the rows)."""
    vol = to_uint8(volume)
    depth = vol.shape[0]
    rows, mags = np.zeros((depth, 96), np.float32), np.zeros((depth, 96), np.float64)
    ft, areas, boxes = case["tumor_slices_from_to"], case["tumor_slices_areas"], case["tumor_slices"]

    def feat(k, j, loop):
        y1, x1, y2, x2 = boxes[j]
        return features(_smooth(vol[k, y1:y2, x1:x2], loop))

    if mode == "train":
        for k in range(depth):
            if k not in case["tumor_slices_index"]:
                continue
            ind = case["tumor_slices_index"].index(k)
            big = [j for j in range(ft[ind], ft[ind + 1]) if areas[j] >= 20]
            vals = [feat(k, j, 0) for j in big]
            loop = 1
            while big and len(vals) < 3:
                vals += [feat(k, j, loop) for j in big]
                loop += 1
            if vals:
                rows[k] = np.mean([v for v, _ in vals], axis=0)
                mags[k] = np.mean([m for _, m in vals], axis=0)
        return rows, mags
    counter = np.zeros((depth,), np.int32)
    for tid, (z1, _, _, z2, _, _) in enumerate(case["tumors"]):
        mid = (z2 - z1 - 1) // 2 + z1
        ind = case["tumor_slices_index"].index(mid)
        for j in range(ft[ind], ft[ind + 1]):
            if case["tumor_slices_tid"][j] == tid:
                if areas[j] < 20:
                    break
                vals = [feat(mid, j, loop) for loop in range(3)]
                rows[z1:z2] += np.tile(np.mean([v for v, _ in vals], axis=0, keepdims=True), (z2 - z1, 1))
                mags[z1:z2] += np.mean([m for _, m in vals], axis=0)
                counter[z1:z2] += 1
                break
    div = np.clip(counter, 1, np.inf)
    rows /= div[:, None]
    return rows, mags / div[:, None]


@functools.lru_cache(maxsize=None)
def fixture():
    """[(volume int16, labels uint8, meta record, train rows, eval rows)] recorded from the reference."""
    z = np.load(GOLDEN)
    return tuple((z["vol_%d" % i], z["lab_%d" % i], json.loads(z["meta_%d" % i].tobytes().decode()), z["train_%d" % i],
                  z["eval_%d" % i]) for i in range(3))


@functools.lru_cache(maxsize=None)
def restated(mode):
    """glcm_rows_numpy of every fixture case, computed once: [(rows, S_f)]."""
    return tuple(glcm_rows_numpy(vol, meta, mode) for vol, _, meta, _, _ in fixture())


def ulps32(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- the tests
def test_fixture_holds_the_cases_it_was_made_for():
    (v0, _, m0, t0, e0), (v1, _, m1, t1, e1), (v2, _, m2, t2, e2) = fixture()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert min(m0["tumor_slices_areas"]) < 20 and not t0[7].any() and t0[1].any()          # the small tumour is skipped
    ft = m1["tumor_slices_from_to"]
    assert max(b - a for a, b in zip(ft, ft[1:])) == 3                                     # three tumours on a slice
    assert np.ptp(to_uint8(v1)[2, 30:40, 30:42]) == 0                                      # a constant box
    assert any(b[3] - b[1] == 1 for b in m2["tumor_slices"])                               # one pixel wide
    assert any(b[0] == 0 and b[3] == 48 for b in m2["tumor_slices"])                       # at the border
    assert m0["tumors"][0][3] > m0["tumors"][1][0]                                         # z-extents overlap: a counter of 2
    assert all(r.shape == (8, 96) and r.dtype == np.float32 for r in (t0, e0, t1, e1, t2, e2))


def test_sliced_counts_equal_the_double_loop():
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (12, 10)):
        patch = rng.integers(0, 256, shape).astype(np.uint8)
        np.testing.assert_array_equal(glcm_counts_numpy(patch), glcm_counts_brute(patch))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_restatement_reproduces_the_reference_rows(mode):
    for (_, _, _, train, ev), (rows, _) in zip(fixture(), restated(mode)):
        ref = train if mode == "train" else ev
        assert rows.dtype == np.float32
        assert ulps32(rows, ref).max() <= 1.0


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_extractor_bookkeeping_on_restated_features(mode):
    """data/extract.py's patch choice and row assembly, fed with the restated features instead of the device's."""
    from boxsegliver_amd.data import extract
    for vol, _, meta, train, ev in fixture():
        patches, groups = extract.glcm_patches(to_uint8(vol), meta, mode)
        assert all(p.dtype == np.uint8 and p.flags.c_contiguous for p in patches)
        feats = np.stack([glcm_features_numpy(p)[0] for p in patches]) if patches else np.zeros((0, 96))
        rows = extract.glcm_rows(feats, groups, vol.shape[0], mode)
        assert rows.dtype == np.float32 and rows.shape == (vol.shape[0], 96)
        assert ulps32(rows, train if mode == "train" else ev).max() <= 1.0


def test_offsets_table():
    from boxsegliver_amd import ops
    got = ops.glcm_offsets()
    assert got.dtype == np.int32 and got.shape == (12, 2)
    assert [tuple(r) for r in got.tolist()] == list(OFFSETS)
    assert [tuple(r) for r in ops.glcm_offsets((2,), (0, 2)).tolist()] == [(0, 2), (2, 0)]
    assert ops.GLCM_PROPERTIES == PROPS


def _flags(**over):
    a = argparse.Namespace(use_context=True, glcm=True, context_list=["hist", "200", "glcm", "96"], glcm_features=None,
                           glcm_distance=[1, 2, 3], glcm_angle=[0., math.pi * 0.25, math.pi * 0.5, math.pi * 0.75],
                           glcm_noise=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_gate_and_its_refusals():
    from boxsegliver_amd.data import lits
    assert lits.parse_context_list(["hist", "200", "glcm", "96"], glcm=True) == [("hist", 200), ("glcm", 96)]
    assert lits.parse_context_list(["glcm", 96], glcm=True) == [("glcm", 96)]
    with pytest.raises(ValueError, match="`glcm` is not supported without --glcm"):
        lits.parse_context_list(["glcm", "96"])
    with pytest.raises(ValueError, match="glcm.*not supported"):
        lits.parse_context_list(["hist", "200", "glcm", "96"], glcm=False)
    with pytest.raises(ValueError, match="96"):
        lits.parse_context_list(["glcm", "48"], glcm=True)
    with pytest.raises(ValueError, match="not supported"):
        lits.parse_context_list(["ct_conv", "64"], glcm=True)
    assert lits.context_list_from_args(_flags()) == [("hist", 200), ("glcm", 96)]
    assert lits.context_list_from_args(_flags(glcm_features=list(PROPS), glcm_noise=True)) == [("hist", 200), ("glcm", 96)]
    with pytest.raises(ValueError, match="without --glcm"):
        lits.context_list_from_args(_flags(glcm=False))
    with pytest.raises(ValueError, match="glcm_distance"):
        lits.context_list_from_args(_flags(glcm_distance=[1, 2]))
    with pytest.raises(ValueError, match="glcm_angle"):
        lits.context_list_from_args(_flags(glcm_angle=[0.]))
    with pytest.raises(ValueError, match="glcm_features"):
        lits.context_list_from_args(_flags(glcm_features=["contrast"]))
    with pytest.raises(ValueError, match="96"):
        lits.context_list_from_args(_flags(context_list=["glcm", "95"]))
    # without --glcm the three flags are not looked at: a hist-only run is as before
    assert lits.context_list_from_args(_flags(glcm=False, context_list=["hist", "200"], glcm_distance=[5])) == [("hist", 200)]


def test_load_context_rows_scales_only_the_hist_columns(tmp_path):
    from boxsegliver_amd.data import lits
    rng = np.random.default_rng(5)
    hist, glcm = rng.random((4, 200)).astype(np.float32), rng.normal(size=(4, 96)).astype(np.float32)
    for name, rows in (("hist", hist), ("glcm", glcm)):
        d = tmp_path / "feat" / name / "train"
        d.mkdir(parents=True)
        np.save(d / "007.npy", rows)
    got = lits.load_context_rows(tmp_path, [{"PID": 7, "size": [4, 8, 8]}], {7: 1}, 6, [("hist", 200), ("glcm", 96)], "train", 20.)
    assert got.dtype == np.float32 and got.shape == (6, 296)
    np.testing.assert_array_equal(got[1:5, :200], hist * np.float32(20.))
    np.testing.assert_array_equal(got[1:5, 200:], glcm)
    assert not got[0].any() and not got[5].any()
    with pytest.raises(FileNotFoundError, match="extract glcm"):
        lits.load_context_rows(tmp_path, [{"PID": 8, "size": [4, 8, 8]}], {8: 0}, 4, [("glcm", 96)], "train", 20.)


def test_noise_scale_vector():
    from boxsegliver_amd.data import lits
    scale = lits.context_noise_scale([("hist", 200), ("glcm", 96)], 0.002)
    assert scale.dtype == np.float64 and scale.shape == (296,)
    assert np.all(scale[:200] == 0.002) and np.all(scale[200:] == 0.)
    guide = lits.ContextGuide(np.zeros((2, 296), np.float32), 1., scale)
    np.testing.assert_array_equal(guide.noise_scale, scale)
    # a hist-only list: the scale stays the float it was, and the vector form draws the same bits as today's expression
    assert lits.ContextGuide(np.zeros((2, 200), np.float32), 1., 0.002).noise_scale == 0.002
    assert isinstance(lits.ContextGuide(np.zeros((2, 200), np.float32), 1., 0.002).noise_scale, float)
    today = np.random.RandomState(11).normal(0., 1., (8, 200)) * 0.002
    now = np.random.RandomState(11).normal(0., 1., (8, 200)) * lits.context_noise_scale([("hist", 200)], 0.002)
    assert today.tobytes() == now.tobytes()
