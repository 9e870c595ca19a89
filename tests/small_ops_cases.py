"""Rows and float64 restatements for the pool, image-feature, context-branch and boundary-weight kernels (csrc/pool.hip, fc.hip,
conv1d.hip, weights.hip): the table behind tests/test_small_ops_host.py and tests/test_gpu_small_ops_paths.py.

The restatements follow the formulas of the kernels' header comments in plain numpy / float64; none carries a kernel's index
arithmetic.  A row is (id, family, parameters); PATHS names every branch of the family with a predicate over the parameters, CAPS
every grid cap with the number of threads a row asks for.  The host test asserts that every path has a row, that every cap has one
row exactly at it and one over it (ragged second pass), and that the exact tier's inputs keep fp32 / bf16 arithmetic exact.

Exact tier: x integers in [-4, 4], w / b eighths in [-1, 1], dy / dp / add integers in [-2, 2], scale in {1/2, 1, 2}, keep in
{1/2, 1/4}.  Bound tier: the same rows with standard normal inputs (avg-pool: uniform [0, 1), the inputs its existing bound of 1e-7
was written for).
"""
import collections
import zlib

import numpy as np

import unetk_rng

SEED = 0x5EED5
FP32S, BF16S = 0, 2
EW_GRID_CAP = 8192 * 256          # pool.hip ew_grid: blocks x 256 threads
EW_BLOCKS_CAP = 4096 * 256        # conv1d.hip ew_blocks
EDT_NORM_CAP = 1024 * 256         # weights.hip edt_normalise_kernel, per image
BOUNDARY_RTOL = 2e-6              # test_gpu_ops.py::test_boundary_weights_match_oracle_incl_single_label_slice
FC_REL = 1e-5                     # test_gpu_gunet.py, FC and conv1d
# spatial_mean_fwd, bound tier: the float32 restatement of the kernel's summation order (four interleaved lanes, each sequential,
# then added, one division) against float64 on the rows' own Gaussian inputs measures at most 4.40e-7 of max |mean| (sm_hw1024_c130: 256 terms
# per lane; test_small_ops_host.py::test_spatial_mean_bound_is_four_times_the_measured_error repeats the measurement).
SPATIAL_MEAN_MEASURED = 4.4e-7
SPATIAL_MEAN_REL = 4 * SPATIAL_MEAN_MEASURED

Row = collections.namedtuple("Row", "id fam p")
ROWS = []


def _row(rid, fam, **p):
    ROWS.append(Row(rid, fam, p))


# ------------------------------------------------------------------ max-pool 2x2: N H W C, x pixel stride / channel offset, add
for _id, _n, _h, _w, _c, _xs, _xo, _add, _as, _ao in [
        ("mp_1win", 3, 2, 2, 4, 4, 0, None, 0, 0),
        ("mp_c24_add", 3, 6, 8, 24, 24, 0, "dense", 24, 0),
        ("mp_slice_addslice", 3, 4, 6, 4, 12, 4, "slice", 12, 8),
        ("mp_c24_slice", 2, 8, 4, 24, 32, 8, None, 0, 0),
        ("mp_blocks5", 3, 16, 16, 24, 24, 0, "slice", 32, 4),
        ("mp_odd_5x7", 3, 5, 7, 4, 8, 4, None, 0, 0),
        ("mp_odd_3x2", 2, 3, 2, 24, 24, 0, None, 0, 0),
        ("mp_cap_at", 1, 2048, 2048, 8, 8, 0, None, 0, 0),
        ("mp_cap_over", 1, 2048, 2050, 8, 8, 0, None, 0, 0)]:
    _row(_id, "mp2", n=_n, h=_h, w=_w, c=_c, xs=_xs, xo=_xo, add=_add, ast=_as, ao=_ao, cap=_id.startswith("mp_cap"))

# ------------------------------------------------------------------ avg-pool, image gradients, sobel, flip, moments
for _id, _n, _h, _w, _c in [("ap_c1_2x2", 2, 2, 2, 1), ("ap_c2", 2, 4, 6, 2), ("ap_c3", 2, 6, 4, 3),
                            ("ap_cap_at", 1, 2048, 2048, 2), ("ap_cap_over", 1, 2048, 2050, 2)]:
    _row(_id, "avg", n=_n, h=_h, w=_w, c=_c)
for _id, _n, _h, _w, _c in [("ig_1x1", 3, 1, 1, 1), ("ig_h1", 3, 1, 5, 3), ("ig_w1", 3, 4, 1, 1), ("ig_c3", 3, 5, 7, 3),
                            ("ig_c1", 3, 6, 5, 1), ("ig_cap_at", 1, 1024, 1024, 2), ("ig_cap_over", 1, 1025, 1024, 2)]:
    _row(_id, "ig", n=_n, h=_h, w=_w, c=_c)
for _id, _n, _h, _w, _c, _ch in [("sb_h2_c1", 3, 2, 5, 1, 0), ("sb_w2_c2_last", 3, 5, 2, 2, 1), ("sb_2x2_c3_first", 3, 2, 2, 3, 0),
                                 ("sb_c2_first", 2, 3, 3, 2, 0), ("sb_c3_last", 3, 5, 7, 3, 2), ("sb_c4_first", 3, 6, 5, 4, 0),
                                 ("sb_c4_last", 2, 4, 4, 4, 3), ("sb_cap_at", 1, 1024, 2048, 1, 0),
                                 ("sb_cap_over", 1, 1025, 2048, 1, 0)]:
    _row(_id, "sobel", n=_n, h=_h, w=_w, c=_c, ch=_ch)
for _id, _n, _h, _w, _c, _fh, _fw, _sc, _acc in [("fl_00", 2, 5, 7, 3, 0, 0, 2.0, 0), ("fl_01_acc", 2, 5, 7, 1, 0, 1, 0.5, 1),
                                                 ("fl_10", 3, 3, 4, 1, 1, 0, 1.0, 0), ("fl_11_acc", 2, 7, 5, 3, 1, 1, 2.0, 1),
                                                 ("fl_10_acc", 1, 4, 3, 3, 1, 0, 0.5, 1), ("fl_11", 1, 1, 1, 1, 1, 1, 1.0, 0),
                                                 ("fl_cap_at", 1, 1024, 1024, 2, 1, 1, 0.5, 1),
                                                 ("fl_cap_over", 1, 1025, 1024, 2, 1, 1, 2.0, 1)]:
    _row(_id, "flip", n=_n, h=_h, w=_w, c=_c, fh=_fh, fw=_fw, scale=_sc, acc=_acc)
for _g, _hw in [(1, 1), (2, 255), (3, 256), (4, 257), (4, 1), (3, 255), (2, 256), (1, 257)]:
    _row("gm_ps_g%d_p%d" % (_g, _hw), "moments", n=3, hw=_hw, g=_g, ps=1)
for _g, _n, _hw in [(1, 3, 85), (2, 3, 86), (3, 3, 1), (4, 1, 256), (2, 1, 257), (4, 3, 85)]:
    _row("gm_all_g%d_p%d" % (_g, _n * _hw), "moments", n=_n, hw=_hw, g=_g, ps=0)

# ------------------------------------------------------------------ spatial mean: N HW C
for _id, _n, _hw, _c in [("sm_hw1_c1", 3, 1, 1), ("sm_hw3_c63", 3, 3, 63), ("sm_hw4_c64", 3, 4, 64), ("sm_hw5_c65", 3, 5, 65),
                         ("sm_hw1024_c130", 3, 1024, 130), ("sm_hw4_c130", 2, 4, 130), ("sm_cap_at", 2, 1024, 1024),
                         ("sm_cap_over", 2, 1024, 1025)]:
    _row(_id, "smean", n=_n, hw=_hw, c=_c)

# ------------------------------------------------------------------ FC: B k n relu bias db dx keep
for _id, _b, _k, _n, _relu, _bias, _db, _dx, _keep in [
        ("fc_n1_k1_b1", 1, 1, 1, 0, True, True, True, None),
        ("fc_n1_relu", 5, 33, 1, 1, True, True, True, None),
        ("fc_n63_keep2", 5, 33, 63, 1, True, True, True, 0.5),
        ("fc_n64_nobias", 5, 1, 64, 1, False, False, True, None),
        ("fc_n65_lin_keep4", 1, 33, 65, 0, True, True, True, 0.25),
        ("fc_n255_nodx", 5, 33, 255, 1, True, True, False, None),
        ("fc_n256_nodb", 5, 1, 256, 1, True, False, True, 0.5),
        ("fc_n257_keep4", 5, 33, 257, 1, True, True, True, 0.25),
        ("fc_sig_n65", 5, 33, 65, 2, True, True, True, None),
        ("fc_sig_n257_nobias", 1, 1, 257, 2, False, False, True, None)]:
    _row(_id, "fc", b=_b, k=_k, n=_n, relu=_relu, bias=_bias, db=_db, dx=_dx, keep=_keep)

# ------------------------------------------------------------------ conv1d: B L Cin Cout k relu bias db dx
for _id, _b, _l, _ci, _co, _k, _relu, _bias, _db, _dx in [
        ("c1_k1_l1", 1, 1, 1, 2, 1, 0, True, True, True),
        ("c1_k3_l1", 3, 1, 8, 2, 3, 1, True, True, True),
        ("c1_k3_l2_nobias", 3, 2, 1, 16, 3, 1, False, False, True),
        ("c1_k3_l37", 3, 37, 8, 16, 3, 1, True, True, True),
        ("c1_k1_l37_nodx", 2, 37, 8, 16, 1, 1, True, True, False),
        ("c1_k3_l37_lin_nodb", 2, 37, 1, 2, 3, 0, True, False, True),
        ("c1_cap_out_at", 128, 128, 1, 64, 3, 1, True, True, True),
        ("c1_cap_out_over", 128, 129, 1, 64, 3, 1, True, True, True),
        ("c1_cap_x_at", 128, 128, 64, 1, 3, 1, True, True, True),
        ("c1_cap_x_over", 128, 129, 64, 1, 3, 1, True, True, True),
        ("c1_cap_w_at", 1, 1, 1024, 1024, 1, 1, True, True, True),
        ("c1_cap_w_over", 1, 1, 1024, 1025, 1, 1, True, True, True)]:
    _row(_id, "conv1d", b=_b, l=_l, ci=_ci, co=_co, k=_k, relu=_relu, bias=_bias, db=_db, dx=_dx)
for _id, _b, _l, _c in [("p1_l1", 1, 1, 1), ("p1_l2", 3, 2, 1), ("p1_l7", 3, 7, 16), ("p1_l8", 3, 8, 16), ("p1_l7_c1", 2, 7, 1),
                        ("p1_cap_at", 128, 256, 64), ("p1_cap_over", 128, 257, 64)]:
    _row(_id, "mp1", b=_b, l=_l, c=_c)

# ------------------------------------------------------------------ boundary weights: N H W, label content
for _id, _n, _h, _w, _kind in [("bw_w1", 3, 9, 1, "random"), ("bw_h1", 3, 1, 9, "random"), ("bw_w257", 2, 5, 257, "blobs"),
                               ("bw_stripes", 2, 6, 40, "stripes"), ("bw_single_between", 3, 8, 12, "single_between"),
                               ("bw_borders", 2, 7, 9, "borders"), ("bw_ringfree", 3, 7, 9, "ringfree"),
                               ("bw_wmax", 1, 2, 12288, "stripes"), ("bw_cap_at", 2, 512, 512, "blobs"),
                               ("bw_cap_over", 2, 513, 512, "blobs")]:
    _row(_id, "boundary", n=_n, h=_h, w=_w, kind=_kind)

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def rows(fam):
    return [r for r in ROWS if r.fam == fam]


# ------------------------------------------------------------------ threads asked of each capped grid
def _quads(p):
    return p["n"] * (p["h"] // 2) * (p["w"] // 2) * (p["c"] // 4)


CAPS = [
    # kernel, family, threads(p), cap
    ("maxpool2_fwd_kernel / maxpool2_bwd_kernel", "mp2", _quads, EW_GRID_CAP),
    ("avgpool2_fwd_kernel", "avg", lambda p: p["n"] * (p["h"] // 2) * (p["w"] // 2) * p["c"], EW_GRID_CAP),
    ("image_gradients_kernel", "ig", lambda p: p["n"] * p["h"] * p["w"] * p["c"], EW_GRID_CAP),
    ("sobel_concat_kernel", "sobel", lambda p: p["n"] * p["h"] * p["w"], EW_GRID_CAP),
    ("flip_axpy_kernel", "flip", lambda p: p["n"] * p["h"] * p["w"] * p["c"], EW_GRID_CAP),
    ("spatial_mean_bwd_kernel", "smean", lambda p: p["n"] * p["hw"] * p["c"], EW_GRID_CAP),
    ("conv1d_fwd_kernel / conv1d_bwd_pre_kernel", "conv1d", lambda p: p["b"] * p["l"] * p["co"], EW_BLOCKS_CAP),
    ("conv1d_bwd_x_kernel", "conv1d", lambda p: p["b"] * p["l"] * p["ci"], EW_BLOCKS_CAP),
    ("conv1d_bwd_w_kernel", "conv1d", lambda p: p["k"] * p["ci"] * p["co"], EW_BLOCKS_CAP),
    ("maxpool1d_fwd_kernel / maxpool1d_bwd_kernel", "mp1", lambda p: p["b"] * ((p["l"] + 1) // 2) * p["c"], EW_BLOCKS_CAP),
    ("edt_normalise_kernel", "boundary", lambda p: p["h"] * p["w"], EDT_NORM_CAP),
]

# ------------------------------------------------------------------ the table of DESIGN.md 6.6: path (predicate), kernel, family
PATHS = [
    ("one quad per pixel (C = 4)", "maxpool2_*_kernel<float|bf16_t>", "mp2", lambda p: p["c"] == 4),
    ("several quads (C = 24)", "maxpool2_*_kernel", "mp2", lambda p: p["c"] == 24),
    ("x a concat slice (x_stride > C, channel offset)", "maxpool2_*_kernel", "mp2", lambda p: p["xs"] > p["c"] and p["xo"] > 0),
    ("add == NULL", "maxpool2_bwd_kernel", "mp2", lambda p: p["add"] is None and p["h"] % 2 == 0 and p["w"] % 2 == 0),
    ("add dense (add_stride == C)", "maxpool2_bwd_kernel", "mp2", lambda p: p["add"] == "dense"),
    ("add a slice (add_stride > C)", "maxpool2_bwd_kernel", "mp2", lambda p: p["add"] == "slice" and p["ast"] > p["c"]),
    ("one window (H = W = 2)", "maxpool2_*_kernel", "mp2", lambda p: p["h"] == 2 and p["w"] == 2),
    ("odd H and W, forward only (VALID)", "maxpool2_fwd_kernel", "mp2", lambda p: p["h"] % 2 == 1 and p["w"] % 2 == 1),
    ("odd H, even W, forward only", "maxpool2_fwd_kernel", "mp2", lambda p: p["h"] % 2 == 1 and p["w"] % 2 == 0),
    ("more than one block below the cap", "maxpool2_*_kernel", "mp2", lambda p: 256 < _quads(p) < EW_GRID_CAP),
    ("C = 1", "avgpool2_fwd_kernel", "avg", lambda p: p["c"] == 1),
    ("C = 2", "avgpool2_fwd_kernel", "avg", lambda p: p["c"] == 2),
    ("C = 3", "avgpool2_fwd_kernel", "avg", lambda p: p["c"] == 3),
    ("one window per image (2 x 2)", "avgpool2_fwd_kernel", "avg", lambda p: p["h"] == 2 and p["w"] == 2 and p["n"] == 2),
    ("H = 1 and W = 1", "image_gradients_kernel", "ig", lambda p: p["h"] == 1 and p["w"] == 1 and p["n"] == 3),
    ("H = 1", "image_gradients_kernel", "ig", lambda p: p["h"] == 1 and p["w"] > 1),
    ("W = 1", "image_gradients_kernel", "ig", lambda p: p["w"] == 1 and p["h"] > 1),
    ("C = 3, N = 3", "image_gradients_kernel", "ig", lambda p: p["c"] == 3 and p["n"] == 3 and p["h"] > 1 and p["w"] > 1),
    ("C = 1, N = 3", "image_gradients_kernel", "ig", lambda p: p["c"] == 1 and p["n"] == 3 and p["h"] > 1 and p["w"] > 1),
    ("H = 2: the reflected row is row 0", "sobel_concat_kernel", "sobel", lambda p: p["h"] == 2),
    ("W = 2", "sobel_concat_kernel", "sobel", lambda p: p["w"] == 2),
] + [("C = %d, ch = %s" % (c, "0" if first else "C - 1"), "sobel_concat_kernel", "sobel",
      (lambda c, first: lambda p: p["c"] == c and p["ch"] == (0 if first else c - 1))(c, first))
     for c in (1, 2, 3, 4) for first in (True, False)] + [
    ("N = 3, distinct images", "sobel_concat_kernel", "sobel", lambda p: p["n"] == 3 and p["h"] > 2 and p["w"] > 2),
] + [("flip_h = %d, flip_w = %d" % (fh, fw), "flip_axpy_kernel", "flip",
      (lambda fh, fw: lambda p: p["fh"] == fh and p["fw"] == fw)(fh, fw)) for fh in (0, 1) for fw in (0, 1)] + [
    ("accumulate", "flip_axpy_kernel", "flip", lambda p: p["acc"] == 1 and p["h"] % 2 == 1 and p["w"] % 2 == 1),
    ("overwrite", "flip_axpy_kernel", "flip", lambda p: p["acc"] == 0 and p["h"] % 2 == 1 and p["w"] % 2 == 1),
    ("C = 1", "flip_axpy_kernel", "flip", lambda p: p["c"] == 1),
    ("C = 3", "flip_axpy_kernel", "flip", lambda p: p["c"] == 3),
] + [("G = %d" % g, "guide_moments_kernel", "moments", (lambda g: lambda p: p["g"] == g)(g)) for g in (1, 2, 3, 4)] + [
    ("P = %d (per sample, N = 3)" % hw, "guide_moments_kernel", "moments",
     (lambda hw: lambda p: p["ps"] == 1 and p["hw"] == hw and p["n"] == 3)(hw)) for hw in (1, 255, 256, 257)] + [
    ("P = %d (whole batch)" % pp, "guide_moments_kernel", "moments",
     (lambda pp: lambda p: p["ps"] == 0 and p["n"] * p["hw"] == pp)(pp)) for pp in (255, 256, 257)] + [
    ("whole batch, N = 3", "guide_moments_kernel", "moments", lambda p: p["ps"] == 0 and p["n"] == 3),
] + [("C = %d" % c, "spatial_mean_fwd_kernel, spatial_mean_bwd_kernel", "smean", (lambda c: lambda p: p["c"] == c and p["n"] == 3)(c))
     for c in (1, 63, 64, 65, 130)] + [
    ("HW = %d" % hw, "spatial_mean_fwd_kernel, spatial_mean_bwd_kernel", "smean", (lambda hw: lambda p: p["hw"] == hw)(hw))
    for hw in (1, 3, 4, 5, 1024)] + [
    ("n = %d" % n, "fc_fwd_kernel, fc_bwd_*_kernel", "fc", (lambda n: lambda p: p["n"] == n and p["relu"] < 2)(n))
    for n in (1, 63, 64, 65, 255, 256, 257)] + [
    ("k = 1", "fc_*_kernel", "fc", lambda p: p["k"] == 1),
    ("k = 33", "fc_*_kernel", "fc", lambda p: p["k"] == 33),
    ("B = 1", "fc_*_kernel", "fc", lambda p: p["b"] == 1),
    ("B = 5", "fc_*_kernel", "fc", lambda p: p["b"] == 5),
    ("relu 0", "fc_fwd_kernel, fc_bwd_pre_kernel", "fc", lambda p: p["relu"] == 0),
    ("relu 1", "fc_fwd_kernel, fc_bwd_pre_kernel", "fc", lambda p: p["relu"] == 1),
    ("relu 2 without a mask (bound tier only)", "fc_fwd_kernel, fc_bwd_pre_kernel", "fc", lambda p: p["relu"] == 2 and p["keep"] is None),
    ("b == NULL", "fc_fwd_kernel", "fc", lambda p: not p["bias"]),
    ("db == NULL", "fc_bwd_pre_kernel", "fc", lambda p: not p["db"]),
    ("db == NULL with a bias", "fc_bwd_pre_kernel", "fc", lambda p: not p["db"] and p["bias"]),
    ("dx == NULL: no fc_bwd_x_kernel", "fc_bwd_pre_kernel, fc_bwd_w_kernel", "fc", lambda p: not p["dx"]),
    ("mask, keep 1/2", "fc_fwd_kernel, fc_bwd_pre_kernel", "fc", lambda p: p["keep"] == 0.5),
    ("mask, keep 1/4", "fc_fwd_kernel, fc_bwd_pre_kernel", "fc", lambda p: p["keep"] == 0.25),
    ("k = 1", "conv1d_*_kernel", "conv1d", lambda p: p["k"] == 1 and p["l"] > 1),
    ("k = 3", "conv1d_*_kernel", "conv1d", lambda p: p["k"] == 3 and p["l"] > 2),
    ("L = 1 (k = 3: the centre tap alone)", "conv1d_*_kernel", "conv1d", lambda p: p["l"] == 1 and p["k"] == 3),
    ("L = 2", "conv1d_*_kernel", "conv1d", lambda p: p["l"] == 2 and p["k"] == 3),
    ("L = 37", "conv1d_*_kernel", "conv1d", lambda p: p["l"] == 37),
    ("Cin = 1", "conv1d_*_kernel", "conv1d", lambda p: p["ci"] == 1),
    ("Cin = 8", "conv1d_*_kernel", "conv1d", lambda p: p["ci"] == 8),
    ("Cout = 2", "conv1d_*_kernel", "conv1d", lambda p: p["co"] == 2),
    ("Cout = 16", "conv1d_*_kernel", "conv1d", lambda p: p["co"] == 16),
    ("b == NULL", "conv1d_fwd_kernel", "conv1d", lambda p: not p["bias"]),
    ("db == NULL", "conv1d_bwd_w_kernel", "conv1d", lambda p: not p["db"]),
    ("dx == NULL: no conv1d_bwd_x_kernel", "conv1d_bwd_pre_kernel, conv1d_bwd_w_kernel", "conv1d", lambda p: not p["dx"]),
    ("relu 0", "conv1d_fwd_kernel, conv1d_bwd_pre_kernel", "conv1d", lambda p: p["relu"] == 0),
    ("relu 1", "conv1d_fwd_kernel, conv1d_bwd_pre_kernel", "conv1d", lambda p: p["relu"] == 1),
] + [("L = %d" % l, "maxpool1d_fwd_kernel, maxpool1d_bwd_kernel", "mp1", (lambda l: lambda p: p["l"] == l)(l)) for l in (1, 2, 7, 8)] + [
    ("C = 1", "maxpool1d_*_kernel", "mp1", lambda p: p["c"] == 1),
    ("C = 16", "maxpool1d_*_kernel", "mp1", lambda p: p["c"] == 16),
    ("W = 1", "edt_columns_kernel, edt_rows_kernel", "boundary", lambda p: p["w"] == 1),
    ("H = 1", "edt_columns_kernel, edt_rows_kernel", "boundary", lambda p: p["h"] == 1),
    ("W = 257: second column of a thread, LDS row", "edt_rows_kernel", "boundary", lambda p: p["w"] == 257),
    ("columns without a ring pixel (G_INF skip)", "edt_rows_kernel", "boundary", lambda p: p["kind"] == "stripes" and p["w"] < 100),
    ("has_ring per image: a single-label image between two others", "edt_rows_kernel", "boundary", lambda p: p["kind"] == "single_between"),
    ("ring pixels on all four borders", "edt_columns_kernel", "boundary", lambda p: p["kind"] == "borders"),
    ("ring-free images: the closed form", "edt_rows_kernel", "boundary", lambda p: p["kind"] == "ringfree"),
    ("W = 12288: 48 KiB LDS row", "edt_rows_kernel", "boundary", lambda p: p["w"] == 12288 and p["h"] == 2),
]


def rows_of(path):
    return [r.id for r in rows(path[2]) if path[3](r.p)]


def cap_rows(cap):
    """(ids exactly at the cap, ids over it) of one CAPS entry."""
    name, fam, threads, limit = cap
    at = [r.id for r in rows(fam) if threads(r.p) == limit]
    over = [r.id for r in rows(fam) if threads(r.p) > limit]
    return at, over


# ------------------------------------------------------------------ helpers
def round_bf16(a):
    """float64 / float32 array -> the bf16 value it rounds to (RNE), as float64."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def store(a, storage):
    return round_bf16(a) if storage == BF16S else f32(a)


def _rng(row, tier):
    return np.random.default_rng(zlib.crc32((row.id + tier).encode()))


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _eighths(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64) / 8.0


def _gauss(rng, shape):
    return f32(rng.standard_normal(shape))


def windows2(x):
    """[N, H, W, C] -> the 2x2 VALID windows in scan order [N, Ho, Wo, 4, C]."""
    n, h, w, c = x.shape
    ho, wo = h // 2, w // 2
    return x[:, :2 * ho, :2 * wo].reshape(n, ho, 2, wo, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, ho, wo, 4, c)


def unwindows2(win, h, w):
    n, ho, wo, _, c = win.shape
    out = np.zeros((n, h, w, c), win.dtype)
    out[:, :2 * ho, :2 * wo] = win.reshape(n, ho, wo, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * ho, 2 * wo, c)
    return out


def _pool_edges(win, skip=None):
    """Edge content of the pool rows, in place on windows [..., K, C] (K = 4 or 2).  The pattern of a (window, channel) pair is its
    running number % 8, counted over the channels other than `skip` (the bf16 tie channel, overwritten afterwards), so that a row
    with eight such pairs carries every pattern:
    0: all equal; 1 .. K: the only maximum at each place; 5 / 6: -0.0 and +0.0 mixed, in both orders; 7: a zero pixel at place
    window % K among non-zero neighbours (with the zeros that are drawn anyway, about one pixel in eight is 0).  Returns the patterns."""
    k, c = win.shape[-2], win.shape[-1]
    lead = win.shape[:-2]
    ceff = c - (skip is not None)
    cidx = np.arange(c) - (0 if skip is None else (np.arange(c) > skip))
    wn = np.arange(int(np.prod(lead))).reshape(lead)[..., None]
    pat = (wn * ceff + cidx) % 8
    pat_k = np.broadcast_to(pat[..., None, :], win.shape)
    place = np.broadcast_to(np.arange(k).reshape((1,) * len(lead) + (k, 1)), win.shape)
    first = np.broadcast_to(win[..., :1, :], win.shape)
    win[...] = np.where(pat_k == 0, first, win)
    for j in range(k):
        sel = pat_k == 1 + j
        win[...] = np.where(sel, np.where(place == j, 4.0, np.minimum(win, 3.0)), win)
    win[...] = np.where(pat_k == 5, np.where(place % 3 == 0, -0.0, 0.0), win)
    win[...] = np.where(pat_k == 6, np.where(place % 3 == 0, 0.0, -0.0), win)
    hole = place == np.broadcast_to((wn % k)[..., None, :], win.shape)
    win[...] = np.where(pat_k == 7, np.where(hole, 0.0, np.where(win == 0, 1.0, win)), win)
    return pat


TIE_WINDOW = (64.25, 64.0, 63.0, 63.5)      # the first window of the bf16 tie channel: 64.25 rounds to 64, a tie that fp32 does not have


def _live(dp, pat):
    """The gradient of the pattern-7 windows is non-zero: their zero pixel sits under a non-zero gradient."""
    return np.where((pat == 7) & (dp == 0), 1.0, dp)


def tile_hw(a, h, w):
    """Repeat a [N, h0, w0, ...] block along H and W and crop to [N, h, w, ...]."""
    reps = (1, -(-h // a.shape[1]), -(-w // a.shape[2])) + (1,) * (a.ndim - 3)
    return np.tile(a, reps)[:, :h, :w]


# ------------------------------------------------------------------ inputs
def make_inputs(row, tier, storage=FP32S):
    """The row's inputs as float64 arrays holding storage-representable values (tier "exact" or "gauss")."""
    p, rng, ex = row.p, _rng(row, tier), tier == "exact"
    draw = (lambda lo, hi, shape: _ints(rng, lo, hi, shape)) if ex else (lambda lo, hi, shape: _gauss(rng, shape))
    a = {}
    if row.fam == "mp2":
        n, h, w, c = p["n"], p["h"], p["w"], p["c"]
        if ex and p["cap"]:
            # 134 MB of payload: a block of 37 x 41 windows (x and dp) with the edge content, repeated (no power of two, so that a
            # pass shifted by the grid's 2^21 quads meets another phase); one input for both storages, the tie channel rounded
            # already.  reference() pools the block and repeats the result: the windows never straddle two blocks.
            win = _ints(rng, -4, 4, (n, 37, 41, 4, c))
            pat = _pool_edges(win, skip=1)
            win[..., 1] = 64.0 + _ints(rng, -4, 4, (n, 37, 41, 4)) / 4.0
            win[:, 0, 0, :, 1] = TIE_WINDOW
            win[..., 1] = round_bf16(win[..., 1])
            a["blk"] = dict(x=unwindows2(win, 74, 82), dp=_live(_ints(rng, -2, 2, (n, 37, 41, c)), pat))
            a["x"], a["dp"], a["add"] = tile_hw(a["blk"]["x"], h, w), tile_hw(a["blk"]["dp"], h // 2, w // 2), None
            return a
        x = draw(-4, 4, (n, h, w, c))
        dp = draw(-2, 2, (n, h // 2, w // 2, c))
        if ex:
            win = windows2(x).copy()
            dp = _live(dp, _pool_edges(win, skip=1 if storage == BF16S else None))
            x[:, :h // 2 * 2, :w // 2 * 2] = unwindows2(win, h // 2 * 2, w // 2 * 2)
            if storage == BF16S:                     # ties that exist only after the rounding to bf16
                x[..., 1] = 64.0 + _ints(rng, -4, 4, (n, h, w)) / 4.0
                x[:, :2, :2, 1] = np.reshape(TIE_WINDOW, (2, 2))
        a["x"] = store(x, storage)
        a["dp"] = store(dp, storage)
        a["add"] = store(draw(-2, 2, (n, h, w, c)), storage) if p["add"] else None
    elif row.fam == "avg":
        shape = (p["n"], p["h"], p["w"], p["c"])
        a["x"] = _ints(rng, -4, 4, shape) if ex else f32(rng.random(shape))
    elif row.fam in ("ig", "sobel"):
        a["x"] = draw(-4, 4, (p["n"], p["h"], p["w"], p["c"]))
    elif row.fam == "flip":
        shape = (p["n"], p["h"], p["w"], p["c"])
        a["x"], a["out0"] = draw(-4, 4, shape), draw(-2, 2, shape)
    elif row.fam == "moments":
        shape = (p["n"], p["hw"], p["g"])
        a["guide"] = _ints(rng, 0, 3, shape) if ex else _gauss(rng, shape)
    elif row.fam == "smean":
        a["x"], a["dy"] = draw(-4, 4, (p["n"], p["hw"], p["c"])), draw(-2, 2, (p["n"], p["c"]))
    elif row.fam == "fc":
        b, k, n = p["b"], p["k"], p["n"]
        a["x"] = draw(-4, 4, (b, k))
        a["w"] = _eighths(rng, (k, n)) if ex else _gauss(rng, (k, n)) / np.sqrt(k)
        a["w"] = f32(a["w"])
        a["b"] = (_eighths(rng, (n,)) if ex else _gauss(rng, (n,))) if p["bias"] else None
        a["dy"] = draw(-2, 2, (b, n))
        if ex:                                       # no output is identically zero, however small the row
            a["x"][0, 0] = a["x"][0, 0] or 3.0
            a["w"][0, n // 2] = a["w"][0, n // 2] or 0.5
            a["dy"][0, n // 2] = a["dy"][0, n // 2] or 2.0
        if p["relu"] == 1 and n > 1:                 # pre-activations exactly 0 under a non-zero dy: columns 0 and n - 1
            for o in {0, n - 1}:
                a["w"][:, o] = 0.0
                if a["b"] is not None:
                    a["b"][o] = 0.0
                a["dy"][:, o] = np.where(a["dy"][:, o] == 0, 1.0, a["dy"][:, o])
        elif p["relu"] == 1:                         # one column: the last sample and the bias are zero, sample 0 is positive
            a["x"][b - 1] = 0.0
            a["b"][0] = 0.0
            a["dy"][b - 1] = np.where(a["dy"][b - 1] == 0, 1.0, a["dy"][b - 1])
            a["x"][0] = np.abs(a["x"][0]) * np.where(a["w"][:, 0] >= 0, 1.0, -1.0)
        a["mask"] = None
        if p["keep"] is not None:
            u = unetk_rng.fc_uniform_host(SEED, np.arange(b * n, dtype=np.uint64)).reshape(b, n)     # element r * n + o
            a["mask"] = np.where(u < np.float32(p["keep"]), 1.0 / p["keep"], 0.0)
    elif row.fam == "conv1d":
        b, l, ci, co, k = p["b"], p["l"], p["ci"], p["co"], p["k"]
        a["x"] = draw(-4, 4, (b, l, ci))
        a["w"] = f32(_eighths(rng, (k, ci, co)) if ex else _gauss(rng, (k, ci, co)) / np.sqrt(k * ci))
        a["b"] = (_eighths(rng, (co,)) if ex else _gauss(rng, (co,))) if p["bias"] else None
        a["dy"] = draw(-2, 2, (b, l, co))
        if ex:                                       # no output is identically zero, however small the row
            a["x"][0, 0, 0] = a["x"][0, 0, 0] or 3.0
            a["w"][(k - 1) // 2, 0, co // 2] = a["w"][(k - 1) // 2, 0, co // 2] or 0.5
            a["dy"][0, 0, co // 2] = a["dy"][0, 0, co // 2] or 2.0
        if p["relu"] == 1 and co > 1:                # pre-activations exactly 0 under a non-zero dy: output channel 0
            a["w"][:, :, 0] = 0.0
            if a["b"] is not None:
                a["b"][0] = 0.0
            a["dy"][:, :, 0] = np.where(a["dy"][:, :, 0] == 0, 1.0, a["dy"][:, :, 0])
        elif p["relu"] == 1:                         # one output channel: sample 0 is zero and so is the bias
            a["x"][0] = 0.0
            a["b"][0] = 0.0
            a["dy"][0] = np.where(a["dy"][0] == 0, 1.0, a["dy"][0])
    elif row.fam == "mp1":
        b, l, c = p["b"], p["l"], p["c"]
        x = draw(-4, 4, (b, l, c))
        if ex and l > 1:
            win = x[:, :l // 2 * 2].reshape(b, l // 2, 2, c).copy()
            _pool_edges(win)
            x[:, :l // 2 * 2] = win.reshape(b, l // 2 * 2, c)
        a["x"], a["dy"] = x, draw(-2, 2, (b, (l + 1) // 2, c))
    elif row.fam == "boundary":
        a["labels"] = boundary_labels(row)
    else:
        raise KeyError(row.fam)
    return a


def boundary_labels(row):
    p = row.p
    n, h, w, kind = p["n"], p["h"], p["w"], p["kind"]
    rng = _rng(row, "labels")
    hh, ww = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "random":
        lab = rng.integers(0, 3, size=(n, h, w))
    elif kind == "blobs":
        lab = np.stack([((hh + 3 * i) // 5 + (ww + i) // 7) % 3 if max(h, w) < 300 else ((hh + 9 * i) // 61 + ww // 67) % 3
                        for i in range(n)])
    elif kind == "stripes":
        period = 10 if w < 100 else 1000
        lab = np.stack([((ww + 3 * i) // period) % 2 for i in range(n)])
    elif kind == "single_between":
        lab = rng.integers(0, 3, size=(n, h, w))
        lab[1] = 2
    elif kind == "borders":                          # one foreign pixel in the middle of each border: ring pixels on all four
        lab = np.zeros((n, h, w), np.int64)
        for i in range(n):
            lab[i, 0, w // 2] = lab[i, h - 1, w // 2 - i] = lab[i, h // 2, 0] = lab[i, h // 2 + i, w - 1] = 1 + i
    elif kind == "ringfree":
        lab = np.stack([np.full((h, w), i) for i in range(n)])
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(lab, dtype=np.int32)


# ------------------------------------------------------------------ float64 restatements, one per entry point
def maxpool2_fwd(x):
    """slim.max_pool2d(x, [2, 2]) VALID: the maximum of each 2x2 window; an odd last row / column is never read."""
    return windows2(x).max(axis=3)


def maxpool2_bwd(x, dp, add=None):
    """TF MaxPoolGrad: the first maximum of the window in scan order takes dp; `add` (the skip gradient) is added afterwards."""
    n, h, w, c = x.shape
    k = np.argmax(windows2(x), axis=3)                               # np.argmax: first maximum; -0.0 == +0.0
    hot = np.arange(4).reshape(1, 1, 1, 4, 1) == k[:, :, :, None, :]
    dx = unwindows2(np.where(hot, dp[:, :, :, None, :], 0.0), h, w)
    return dx if add is None else dx + add


def avgpool2_fwd(x):
    return windows2(x).sum(axis=3) * 0.25


def image_gradients(x):
    """concat(x, x[h + 1] - x[h], x[w + 1] - x[w]); the last row and the last column of the differences are zero."""
    dy, dx = np.zeros_like(x), np.zeros_like(x)
    dy[:, :-1] = x[:, 1:] - x[:, :-1]
    dx[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    return np.concatenate((x, dy, dx), axis=-1)


def sobel_concat(x, ch):
    """concat(x, dy, dx): 3x3 Sobel cross-correlations of channel ch over the REFLECT-padded image."""
    n, h, w, _ = x.shape
    xp = np.pad(x[..., ch], ((0, 0), (1, 1), (1, 1)), mode="reflect")
    ky = np.array([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]])
    dy, dx = np.zeros((n, h, w)), np.zeros((n, h, w))
    for i in range(3):
        for j in range(3):
            dy += ky[i, j] * xp[:, i:i + h, j:j + w]
            dx += ky[j, i] * xp[:, i:i + h, j:j + w]
    return np.concatenate((x, dy[..., None], dx[..., None]), axis=-1)


def flip_axpy(x, out0, fh, fw, scale, acc):
    v = x[:, ::-1] if fh else x
    v = v[:, :, ::-1] if fw else v
    return scale * v + (out0 if acc else 0.0)


def guide_moments(guide, per_sample):
    """[groups][G + G * G]: the means of g_i, then of g_i * g_j at G + i * G + j, over the group's pixels."""
    n, hw, g = guide.shape
    grp = guide if per_sample else guide.reshape(1, n * hw, g)
    second = np.einsum("qpi,qpj->qij", grp, grp) / grp.shape[1]
    return np.concatenate((grp.mean(axis=1), second.reshape(grp.shape[0], g * g)), axis=1)


def spatial_mean_fwd(x):
    return x.sum(axis=1) / x.shape[1]


def spatial_mean_bwd(dy, hw):
    return np.repeat(dy[:, None, :], hw, axis=1) / hw


def spatial_mean_fwd_f32(x):
    """float32 restatement of the kernel's summation order: four interleaved pixel lanes, each sequential, then added, one division."""
    x = x.astype(np.float32)
    lanes = []
    for pl in range(4):
        s = np.zeros((x.shape[0], x.shape[2]), np.float32)
        for q in range(pl, x.shape[1], 4):
            s = s + x[:, q]
        lanes.append(s)
    return (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]) / np.float32(x.shape[1])


def spatial_mean_bwd_f32(dy, hw):
    """The two roundings of the kernel: inv = float32(1 / HW), then dy * inv."""
    inv = np.float32(1.0) / np.float32(hw)
    return np.repeat((dy.astype(np.float32) * inv)[:, None, :], hw, axis=1).astype(np.float64)


def _act(pre, relu):
    if relu == 1:
        return np.maximum(pre, 0.0)
    if relu == 2:
        return 1.0 / (1.0 + np.exp(-pre))
    return pre


def _gate(d, pre, relu, ge=False):
    if relu == 1:
        return d * ((pre >= 0) if ge else (pre > 0))
    if relu == 2:
        s = _act(pre, 2)
        return d * s * (1.0 - s)
    return d


def fc(a, relu, ge=False):
    """act(x @ w + b) * mask and its gradients; ge = the WRONG gate (>= 0) that each ReLU row must tell apart."""
    x, w, m = a["x"], a["w"], a["mask"]
    pre = x @ w + (a["b"] if a["b"] is not None else 0.0)
    y = _act(pre, relu) * (m if m is not None else 1.0)
    d = _gate(a["dy"] * (m if m is not None else 1.0), pre, relu, ge)
    return dict(pre=pre, y=y, dpre=d, db=d.sum(axis=0), dw=x.T @ d, dx=d @ w.T)


def conv1d(a, k, relu, ge=False):
    """slim.conv1d SAME, pad = (k - 1) / 2, w = TF [k, Cin, Cout]."""
    x, w = a["x"], a["w"]
    b, l, ci = x.shape
    pad = (k - 1) // 2
    xp = np.pad(x, ((0, 0), (pad, pad), (0, 0)))
    pre = sum(xp[:, t:t + l] @ w[t] for t in range(k)) + (a["b"] if a["b"] is not None else 0.0)
    d = _gate(a["dy"], pre, relu, ge)
    dw = np.stack([np.einsum("blc,blo->co", xp[:, t:t + l], d) for t in range(k)])
    dxp = np.zeros_like(xp)
    for t in range(k):
        dxp[:, t:t + l] += d @ w[t].T
    return dict(pre=pre, y=_act(pre, relu), dpre=d, db=d.sum(axis=(0, 1)), dw=dw, dx=dxp[:, pad:pad + l])


def _windows1(x):
    b, l, c = x.shape
    lo = (l + 1) // 2
    xp = np.concatenate((x, np.full((b, 2 * lo - l, c), -np.inf)), axis=1)
    return xp.reshape(b, lo, 2, c)


def maxpool1d_fwd(x):
    """max_pooling1d(2, 2, "same"): Lo = ceil(L / 2); the last window of an odd L holds one element."""
    return _windows1(x).max(axis=2)


def maxpool1d_bwd(x, dy):
    win = _windows1(x)
    hot = np.arange(2).reshape(1, 1, 2, 1) == np.argmax(win, axis=2)[:, :, None, :]
    return np.where(hot, dy[:, :, None, :], 0.0).reshape(x.shape[0], -1, x.shape[2])[:, :x.shape[1]]


def boundary_weights(labels):
    import torch
    from oracle import losses
    lab = torch.from_numpy(np.asarray(labels)).long()
    return losses.compute_weights("boundary", lab, int(lab.max()) + 1).numpy().astype(np.float64)


def boundary_ringfree_unscaled(h, w):
    """A single-label image: d = float32(sqrt((h + 1)^2 + w^2)) (scipy's no-background convention), exp(-d / 25) + 1."""
    hh, ww = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.sqrt((hh + 1) ** 2 + ww ** 2).astype(np.float32).astype(np.float64)
    return np.exp(-d / 25.0) + 1.0


def boundary_ws_bytes(n, h, w):
    """include/unetk.h: the column distances [N][H][W], the row sums [N][H], the ring flags [N] and 64 spare words."""
    return (n * h * w + n * h + n + 64) * 4


def reference(row, a, storage=FP32S):
    """Every output of the row's entry points in float64 (under bf16 storage: before the one rounding of stored values)."""
    p, f = row.p, row.fam
    if f == "mp2" and "blk" in a:
        blk = a["blk"]
        return dict(p=tile_hw(maxpool2_fwd(blk["x"]), p["h"] // 2, p["w"] // 2), dx=tile_hw(maxpool2_bwd(blk["x"], blk["dp"]), p["h"], p["w"]))
    if f == "mp2":
        out = dict(p=maxpool2_fwd(a["x"]))
        if p["h"] % 2 == 0 and p["w"] % 2 == 0:
            out["dx"] = maxpool2_bwd(a["x"], a["dp"], a["add"])
        return out
    if f == "avg":
        return dict(p=avgpool2_fwd(a["x"]))
    if f == "ig":
        return dict(out=image_gradients(a["x"]))
    if f == "sobel":
        return dict(out=sobel_concat(a["x"], p["ch"]))
    if f == "flip":
        return dict(out=flip_axpy(a["x"], a["out0"], p["fh"], p["fw"], p["scale"], p["acc"]))
    if f == "moments":
        return dict(out=guide_moments(a["guide"], p["ps"]))
    if f == "smean":
        return dict(y=spatial_mean_fwd(a["x"]), dx=spatial_mean_bwd(a["dy"], p["hw"]))
    if f == "fc":
        return fc(a, p["relu"])
    if f == "conv1d":
        return conv1d(a, p["k"], p["relu"])
    if f == "mp1":
        return dict(y=maxpool1d_fwd(a["x"]), dx=maxpool1d_bwd(a["x"], a["dy"]))
    if f == "boundary":
        return dict(wmap=boundary_weights(a["labels"]))
    raise KeyError(f)


def exact_tier(row):
    """Rows whose exact tier exists: the sigmoid is no exact function, the boundary map has a tolerance in every tier."""
    return row.fam != "boundary" and not (row.fam == "fc" and row.p["relu"] == 2)


def storages(row):
    return (FP32S, BF16S) if row.fam == "mp2" else (FP32S,)


# ------------------------------------------------------------------ exactness conditions of the exact tier
def exact_sums(row, a):
    """[(name, unit, sum of the summands' magnitudes / unit, integer factors, factors that are multiples of the unit)] for every
    sum the row's kernels form: a summand is a product of integer factors and at most one multiple of the unit."""
    p, f = row.p, row.fam
    ab = np.abs
    if f == "mp2":
        return [] if a["add"] is None else [("dx = route + add", 1.0, float(ab(a["dp"]).max() + ab(a["add"]).max()), [a["dp"], a["add"]], [])]
    if f == "avg":
        return [("window sum", 1.0, float(windows2(ab(a["x"])).sum(axis=3).max()), [a["x"]], [])]
    if f == "ig":
        return [("difference", 1.0, 2 * float(ab(a["x"]).max()), [a["x"]], [])]
    if f == "sobel":
        return [("sobel", 1.0, 8 * float(ab(a["x"]).max()), [a["x"]], [])]
    if f == "flip":
        return [("axpy", 0.5, float((p["scale"] * ab(a["x"]) + ab(a["out0"])).max()) / 0.5, [], [p["scale"] * a["x"], a["out0"]])]
    if f == "moments":
        g = a["guide"] if p["ps"] else a["guide"].reshape(1, -1, p["g"])
        return [("sum g_i g_j", 1.0, float(np.einsum("qpi,qpj->qij", ab(g), ab(g)).max()), [g], [])]
    if f == "smean":
        return [("pixel sum", 1.0, float(ab(a["x"]).sum(axis=1).max()), [a["x"]], [])]
    if f == "fc":
        m = a["mask"] if a["mask"] is not None else 1.0
        d = a["dy"] * m
        bias = [a["b"]] if a["b"] is not None else []
        r = fc(dict(x=ab(a["x"]), w=ab(a["w"]), b=ab(a["b"]) if bias else None, dy=ab(d), mask=None), 0)
        return [("pre", 1 / 8, float(r["pre"].max()) * 8, [a["x"]], [a["w"]] + bias), ("db", 1.0, float(r["db"].max()), [d], []),
                ("dw", 1.0, float(r["dw"].max()), [a["x"], d], []), ("dx", 1 / 8, float(r["dx"].max()) * 8, [d], [a["w"]])]
    if f == "conv1d":
        bias = [a["b"]] if a["b"] is not None else []
        r = conv1d(dict(x=ab(a["x"]), w=ab(a["w"]), b=ab(a["b"]) if bias else None, dy=ab(a["dy"])), p["k"], 0)
        return [("pre", 1 / 8, float(r["pre"].max()) * 8, [a["x"]], [a["w"]] + bias), ("db", 1.0, float(r["db"].max()), [a["dy"]], []),
                ("dw", 1.0, float(r["dw"].max()), [a["x"], a["dy"]], []), ("dx", 1 / 8, float(r["dx"].max()) * 8, [a["dy"]], [a["w"]])]
    if f == "mp1":
        return []
    raise KeyError(f)
