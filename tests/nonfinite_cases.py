"""Rows, receptive-field sets and float64 restatements of the non-finite tier: the table behind tests/test_nonfinite_host.py
(no GPU) and tests/test_gpu_nonfinite.py (include/unetk.h, "Non-finite values on the forward path").

A row takes the exact-tier inputs of an existing path row (`src`, through that family's own generator: small_ops_cases.py,
norm_paths.py, test_gpu_conv_paths.py, test_gpu_conv_epilogue_paths.py, test_gpu_deconv_paths.py, conv3d_bf16_cases.py),
names one operand and one to three of its elements, and puts a NaN there.  The expected NaN pattern does NOT come from a library
evaluation of the poisoned inputs (how a zero halo meets a NaN filter tap differs between implementations); it comes from two
indicator sets per output, written out from the op's index arithmetic:

  R   the outputs whose in-image receptive field holds a poisoned element: each of them MUST be NaN;
  A   R plus the outputs that meet the poison only through the zero halo (a NaN filter tap that lands outside the image,
      a depth tap skipped at the volume edge, a padded output channel of a live-mask row): they MAY be NaN.

The device test asserts R <= isnan(got) <= A and, outside A, the float64 result of the CLEAN inputs under the row's existing
rule (bit for bit: every row here is of the exact tier; bf16 storage: float64 rounded once).  The host test holds the table
honest: R is not empty, R <= A, at least a quarter of the main output lies outside A, and a float64 restatement of the op
(torch / numpy, the one the family's path test already uses) is NaN on a set between R and A.

The NaN itself comes in two bit patterns (PAYLOADS): the quiet 0x7FC00000 and the low-payload 0x7F800001, whose upper 16 bits are
those of +Inf -- a bf16 store that truncated instead of rounding would write Inf.  Operands that live as bf16 (UNETK_BF16S
activations) take the 16-bit patterns 0x7FC0 and 0x7F81.
"""
import collections

import numpy as np
import torch

import conv3d_bf16_cases as C3
import norm_paths as NP
import small_ops_cases as S
import test_gpu_conv_epilogue_paths as EP
import test_gpu_conv_paths as CP
import test_gpu_deconv_paths as DP
from oracle import tf_ops

FP32, BF16, BF16S = 0, 1, 2
PAYLOADS = ((0x7FC00000, 0x7FC0), (0x7F800001, 0x7F81))         # (fp32 bits, bf16 bits) of the two poisons

Row = collections.namedtuple("Row", "id fam src prec operand pos opt")
ROWS = []


def _row(rid, fam, src, operand, pos, prec=FP32, **opt):
    pos = [tuple(p) if isinstance(p, (tuple, list)) else (p,) for p in pos]
    assert 1 <= len(pos) <= 3, rid
    ROWS.append(Row(rid, fam, src, prec, operand, pos, opt))


# ------------------------------------------------------------------ pools (small_ops_cases.py rows)
for _k, (_dh, _dw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):          # the NaN at each of the four window places in turn
    _row("mp2_place%d" % _k, "mp2", "mp_c24_add", "x", [(1, 2 + _dh, 4 + _dw, 5)])
    _row("mp2_place%d_bf16s" % _k, "mp2", "mp_c24_add", "x", [(1, 2 + _dh, 4 + _dw, 5)], prec=BF16S)
_row("mp2_three_windows", "mp2", "mp_blocks5", "x", [(0, 0, 0, 0), (1, 7, 9, 23), (2, 15, 15, 12)])
_row("mp2_slice_bf16s", "mp2", "mp_slice_addslice", "x", [(2, 3, 5, 3)], prec=BF16S)
_row("mp1_first", "mp1", "p1_l7", "x", [(0, 2, 3)])
_row("mp1_second", "mp1", "p1_l7", "x", [(1, 3, 5)])
_row("mp1_odd_tail", "mp1", "p1_l7", "x", [(2, 6, 7)])                       # the last window of an odd L holds one element
_row("mp1_l8_last", "mp1", "p1_l8", "x", [(1, 7, 0), (1, 0, 15)])
_row("avg_c3", "avg", "ap_c3", "x", [(1, 3, 2, 1)])
_row("smean_c65", "smean", "sm_hw5_c65", "x", [(1, 3, 64)])
_row("smean_hw1024", "smean", "sm_hw1024_c130", "x", [(2, 1023, 0), (0, 1, 129)])
_row("moments_ps", "moments", "gm_ps_g2_p255", "guide", [(1, 100, 0)])
_row("moments_all", "moments", "gm_all_g4_p255", "guide", [(2, 84, 3)])

# ------------------------------------------------------------------ context branch: fc and conv1d
_row("fc_x_masked", "fc", "fc_n63_keep2", "x", [(2, 7)])                      # dropped units (mask 0) follow the restatement: NaN * 0
_row("fc_w_masked", "fc", "fc_n63_keep2", "w", [(7, 10)])
_row("fc_b_masked", "fc", "fc_n63_keep2", "b", [(10,)])
_row("fc_x_relu", "fc", "fc_n255_nodx", "x", [(0, 0), (4, 32)])
_row("fc_w_lin", "fc", "fc_n65_lin_keep4", "w", [(32, 64)])
_row("c1d_x_edge", "conv1d", "c1_k3_l37", "x", [(1, 0, 2)])
_row("c1d_x_mid", "conv1d", "c1_k3_l37", "x", [(0, 36, 7), (2, 18, 0)])
_row("c1d_w_tap0", "conv1d", "c1_k3_l37", "w", [(0, 3, 5)])                  # tap 0 reads l - 1: outside the row at l = 0
_row("c1d_w_tap2", "conv1d", "c1_k3_l37", "w", [(2, 0, 15)])
_row("c1d_b", "conv1d", "c1_k3_l37", "b", [(5,)])
_row("c1d_k1_x", "conv1d", "c1_k1_l37_nodx", "x", [(1, 36, 0)])

# ------------------------------------------------------------------ norm apply (+ ReLU, + pool): norm_paths.py rows
for _src, _tag in (("map_c24_bn", "bn"), ("map_c24_in", "in"), ("t_g2_plain", "guide"), ("t_g1_d", "density"), ("t_g2_l", "leaky"),
                   ("t_g1_post", "post"), ("t_drop_plain", "drop"), ("t_drop_post", "drop_post"), ("t_gbare_plain", "postshift")):
    _r = NP.BY_ID[_src]
    _p = (_r.n - 1, _r.hw // 2, 5)
    _row("norm_y_" + _tag, "norm", _src, "y", [_p])
    _row("norm_y_" + _tag + "_bf16s", "norm", _src, "y", [_p], prec=BF16S)
_row("norm_scale_bn", "norm", "map_c24_bn", "scale", [(0, 7)])                # what finalize leaves behind a NaN statistic
_row("norm_shift_bn", "norm", "map_c24_bn", "shift", [(0, 7)])
_row("norm_scale_in", "norm", "map_c24_in", "scale", [(1, 7)])
_row("norm_shift_in_bf16s", "norm", "map_c24_in", "shift", [(1, 7)], prec=BF16S)
_row("norm_scale_tail", "norm", "tail_p65_bn", "scale", [(0, 63)])
_row("norm_den", "norm", "t_g1_d", "den", [(1, 9)])
_row("norm_gw", "norm", "t_g2_plain", "gw", [(0, 1, 9)])
for _k in range(4):                                                           # fused apply + ReLU + pool: each window place
    _row("normpool_place%d" % _k, "normpool", "pool_8x8_dskip", "y", [(1, 8 * (2 + _k // 2) + 4 + _k % 2, 9)])
    _row("normpool_place%d_bf16s" % _k, "normpool", "pool_8x8_dskip", "y", [(1, 8 * (2 + _k // 2) + 4 + _k % 2, 9)], prec=BF16S)
_row("normpool_in_scale", "normpool", "pool_6x2_in_n3", "scale", [(2, 11)])
_row("normpool_bn_shift_bf16s", "normpool", "pool_2x6_bn_n3", "shift", [(0, 11)], prec=BF16S)

# ------------------------------------------------------------------ conv3x3 forward with statistics: test_gpu_conv_paths.py rows
_row("c3x3_tiled_x_corner", "conv", "t4_ragged", "x", [(1, 3, 15, 7)])       # corner of a 4 x 16 tile: in three neighbours' halos
_row("c3x3_tiled_x_three", "conv", "t4_ragged", "x", [(0, 21, 39, 0), (1, 8, 16, 31), (1, 0, 0, 16)])
_row("c3x3_tiled_w_tap00", "conv", "t4_ragged", "w", [(0, 0, 5, 9)])
_row("c3x3_tiled_w_tap22", "conv", "t4_ragged", "w", [(2, 2, 31, 127)])
_row("c3x3_bf16_x", "conv", "t4_ragged", "x", [(1, 3, 15, 7)], prec=BF16)
_row("c3x3_bf16_w", "conv", "t4_ragged", "w", [(0, 2, 5, 9)], prec=BF16)
_row("c3x3_lin_x", "conv", "lin_p45", "x", [(3, 4, 2, 10), (6, 8, 4, 63)])
_row("c3x3_lin_w", "conv", "lin_p45", "w", [(2, 0, 3, 7)])
_row("c3x3_bf16s_x", "conv", "lin_p45", "x", [(3, 4, 2, 10)], prec=BF16S)
_row("c3x3_bf16s_w", "conv", "lin_p45", "w", [(2, 0, 3, 7)], prec=BF16S)
_row("c3x3_sk_x", "conv", "sk64", "x", [(1, 7, 7, 1000)])                     # stream-K pieces + lin_sk_fixup
_row("c3x3_sk_w", "conv", "sk64", "w", [(1, 1, 512, 100)])                    # the centre tap never meets the halo: A == R
_row("c3x3_sk128_x", "conv", "sk128", "x", [(7, 15, 0, 255)])
_row("c3x3_c3_ci1_x", "conv", "c3_ci1", "x", [(1, 0, 0, 0)])
_row("c3x3_c3_ci1_w", "conv", "c3_ci1", "w", [(2, 1, 0, 13)])
_row("c3x3_c3_ci3_x", "conv", "c3_ci3", "x", [(0, 12, 20, 2)])
_row("c3x3_direct_ci1_x", "conv", "direct_ci1_co32", "x", [(0, 8, 16, 0)])
_row("c3x3_direct_ci1_w", "conv", "direct_ci1_co32", "w", [(0, 2, 0, 31)])
_row("c3x3_direct_ci3_x", "conv", "direct_ci3_co32", "x", [(0, 4, 7, 1)])
_row("c3x3_direct_ci3_w", "conv", "direct_ci3_co32", "w", [(1, 0, 2, 0)])

# ------------------------------------------------------------------ fused epilogues: test_gpu_conv_epilogue_paths.py AFF rows
_row("aff_t4_x_pool", "aff", "aff_t4", "x", [(1, 3, 15, 7)], pool=True)
_row("aff_t4_scale_pool", "aff", "aff_t4", "scale", [(9,)], pool=True)
_row("aff_t4_shift", "aff", "aff_t4", "shift", [(9,)], pool=False)
_row("aff_t4_w_pool", "aff", "aff_t4", "w", [(0, 0, 5, 9)], pool=True)
_row("aff_n64_bias_x_pool", "aff", "aff_n64", "x", [(0, 19, 39, 31)], pool=True, bias_only=True)     # --without_norm: scale == 1
_row("aff_n64_bias_shift", "aff", "aff_n64", "shift", [(63,)], pool=False, bias_only=True)
_row("aff_lin_x", "aff", "aff_lin64", "x", [(0, 7, 15, 0)], pool=False)
_row("aff_lin_shift", "aff", "aff_lin64", "shift", [(127,)], pool=False)
_row("aff_sk_x", "aff", "aff_lin_sk", "x", [(5, 0, 8, 64)], pool=False)
_row("aff_sk_scale", "aff", "aff_lin_sk", "scale", [(0,)], pool=False)
_row("aff_c3_ci3_x", "aff", "aff_c3_ci3", "x", [(1, 23, 0, 2)], pool=False)
_row("aff_c3_ci3_shift", "aff", "aff_c3_ci3", "shift", [(33,)], pool=False)
_row("aff_c3_ci1_bs_x", "aff", "aff_c3_ci1_bs", "x", [(0, 11, 17, 0)], prec=BF16S, pool=False)       # fp32 image in, bf16 out
_row("aff_c3_ci1_bs_scale", "aff", "aff_c3_ci1_bs", "scale", [(33,)], prec=BF16S, pool=False)
_row("aff_v3_x_pool", "aff", "aff_bs_v3_64", "x", [(3, 20, 100, 9)], prec=BF16S, pool=True)
_row("aff_v3_shift", "aff", "aff_bs_v3_64", "shift", [(9,)], prec=BF16S, pool=False)

# ------------------------------------------------------------------ transposed convs: test_gpu_deconv_paths.py rows
_row("dc_x", "deconv", "g128_small", "x", [(1, 0, 2, 3, 100)])
_row("dc_w", "deconv", "g128_small", "w", [(0, 1, 0, 9, 50)])
_row("dc_b", "deconv", "g128_small", "b", [(9,)])
_row("dc_x_bf16", "deconv", "g128_small", "x", [(0, 0, 0, 0, 0), (1, 0, 3, 7, 127)], prec=BF16)
_row("dc_w_bf16", "deconv", "g128_small", "w", [(0, 0, 1, 63, 127)], prec=BF16)
_row("dc_x_bf16s", "deconv", "g128_small", "x", [(1, 0, 2, 3, 100)], prec=BF16S)
_row("dc_b_bf16s", "deconv", "g128_small", "b", [(9,)], prec=BF16S)
_row("dc_geo_x", "deconv", "geo_three", "x", [(1, 0, 2, 4, 64)])              # neighbours on both sides of the written slice
_row("dc_geo_w_bf16s", "deconv", "geo_three", "w", [(0, 1, 1, 0, 0)], prec=BF16S)
_row("dc3d_x", "deconv", "g3d_w2_kd2", "x", [(1, 2, 1, 0, 33)])
_row("dc3d_w", "deconv", "g3d_w2_kd2", "w", [(1, 0, 1, 31, 0)])
_row("dc3d_x_bf16", "deconv", "g3d_w2_kd2", "x", [(0, 0, 0, 1, 63)], prec=BF16)
_row("dc3d_b", "deconv", "geo_3d_bias", "b", [(20,)])
_row("dc3d_b_bf16", "deconv", "geo_3d_bias", "b", [(31,)], prec=BF16)

# ------------------------------------------------------------------ conv3d forward with statistics
# fp32: src = index into test_gpu_ops3d.CASES ("live": LIVE_CASES), the forward launches as its EXACT_TRACES records them;
# UNETK_BF16: conv3d_bf16_cases.py rows.  x [N, D, H, W, Cin], w [kd, 3, 3, Cin, Cout]
_row("c3d_pertap_w_tap0", "conv3d", 3, "w", [(0, 1, 1, 9, 5)])               # per-tap accumulation: the NaN comes with depth tap 0 only,
_row("c3d_pertap_x", "conv3d", 3, "x", [(1, 0, 7, 15, 63)])                  # and the taps behind it add finite planes onto it
_row("c3d_fused_lin_x", "conv3d", 8, "x", [(1, 7, 11, 0, 1)])
_row("c3d_fused_lin_w_tap2", "conv3d", 8, "w", [(2, 0, 2, 63, 127)])
_row("c3d_s2lin_x", "conv3d", 4, "x", [(0, 4, 7, 7, 10)])                     # s2d_kernel + grouped taps, stride (1, 2, 2)
_row("c3d_s2lin_w", "conv3d", 4, "w", [(0, 2, 2, 10, 100)])
_row("c3d_s2_tiled_odd_x", "conv3d", 2, "x", [(0, 1, 14, 16, 31)])            # odd extents: SAME pads one before
_row("c3d_bridge_s222_x", "conv3d", 5, "x", [(0, 5, 7, 15, 0)])
# the stride-1 conv into scratch + subsample2_stats_kernel (Cout % 64 != 0): the shape of test_gpu_norm_stats.py `subsample_s2`
# and test_gpu_guard_bands.py `subsample_fallback`.  Only the strided outputs count: the NaN of a discarded stride-1 position
# must reach neither y nor the statistics
_SUB = ((1, 2, 8, 12, 32, 32, 1, (1, 2, 2)), ("conv3x3_igemm_kernel<4,1,2,1,1,1,0>", "subsample2_stats_kernel"))
_row("c3d_subsample_x_odd", "conv3d", _SUB[0], "x", [(0, 1, 3, 5, 7)], trace=_SUB[1])       # the centre of one output, 8 discarded
_row("c3d_subsample_x_even", "conv3d", _SUB[0], "x", [(0, 0, 4, 6, 0)], trace=_SUB[1])      # between four outputs
_row("c3d_subsample_w_tap00", "conv3d", _SUB[0], "w", [(0, 0, 0, 3, 9)], trace=_SUB[1])     # reads 2 o: always inside
_row("c3d_subsample_w_tap22", "conv3d", _SUB[0], "w", [(0, 2, 2, 31, 31)], trace=_SUB[1])   # reads 2 o + 2: the halo at the far edge
_row("c3d_live_x", "conv3d", 1, "x", [(0, 3, 12, 12, 5)], live=True)          # a live channel; the padded outputs may be NaN or finite
_row("c3d_bf16_ft_w_tap0", "conv3d", "ft_128_small", "w", [(0, 1, 1, 3, 7)], prec=BF16)      # depth 0 skips tap 0: in A, not in R
_row("c3d_bf16_ft_w_tap2", "conv3d", "ft_256x64_d2", "w", [(2, 0, 0, 31, 63)], prec=BF16)    # D = 2: the last plane skips tap 2
_row("c3d_bf16_ft_x_edge", "conv3d", "ft_128_small", "x", [(1, 2, 6, 12, 63)], prec=BF16)
_row("c3d_bf16_k1_x", "conv3d", "k1_64x32", "x", [(0, 1, 4, 18, 0)], prec=BF16)

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
MAIN = {"conv3d": "y","mp2": "p", "mp1": "y", "avg": "p", "smean": "y", "moments": "out", "fc": "y", "conv1d": "y", "norm": "z", "normpool": "z",
        "conv": "y", "aff": "z", "deconv": "up"}


def rows(fam):
    return [r for r in ROWS if r.fam == fam]


# ------------------------------------------------------------------ helpers
def _mask(shape, *index):
    m = np.zeros(shape, bool)
    if index:
        m[index] = True
    return m


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _np64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def poisoned(case, row=None):
    """The case's inputs with a float64 NaN at the row's elements (the restatements' side; the device side sets bit patterns)."""
    row = row or case["row"]
    out = dict(case["inputs"])
    a = np.array(out[row.operand], np.float64, copy=True)
    for p in row.pos:
        a[p] = np.nan
    out[row.operand] = a
    return out


def _neigh(lo, n):
    return slice(max(lo - 1, 0), min(lo + 2, n))


def _conv_sets(shape_y, row, h, w):
    """3 x 3 SAME conv, y [N, H, W, Cout]: (R, A) of a poisoned x element (n, h, w, ci) or filter tap (kh, kw, ci, co)."""
    R, A = _mask(shape_y), _mask(shape_y)
    for p in row.pos:
        if row.operand == "x":
            R[p[0], _neigh(p[1], h), _neigh(p[2], w), :] = True
        else:
            kh, kw, _, co = p                               # output (oh, ow) reads input (oh + kh - 1, ow + kw - 1)
            R[:, max(1 - kh, 0):min(h + 1 - kh, h), max(1 - kw, 0):min(w + 1 - kw, w), co] = True
            A[..., co] = True
    return R, A | R


def _win_any(m):
    n, h, w, c = m.shape
    return m[:, :h // 2 * 2, :w // 2 * 2].reshape(n, h // 2, 2, w // 2, 2, c).any((2, 4))


# ------------------------------------------------------------------ families: inputs, sets, clean reference, restatement
def _small(row):
    src = S.BY_ID[row.src]
    p, f = src.p, row.fam
    a = S.make_inputs(src, "exact", S.BF16S if row.prec == BF16S else S.FP32S)
    ref = S.reference(src, a, S.BF16S if row.prec == BF16S else S.FP32S)
    outs = collections.OrderedDict()
    if f == "mp2":
        sh = ref["p"].shape
        R = _mask(sh)
        for n, h, w, c in row.pos:
            assert h < p["h"] // 2 * 2 and w < p["w"] // 2 * 2
            R[n, h // 2, w // 2, c] = True
        outs["p"] = (R, R, ref["p"])
        fn = lambda q: dict(p=S.maxpool2_fwd(q["x"]))
    elif f == "mp1":
        R = _mask(ref["y"].shape)
        for b, l, c in row.pos:
            R[b, l // 2, c] = True
        outs["y"] = (R, R, ref["y"])
        fn = lambda q: dict(y=_maxpool1d_nan(q["x"]))
    elif f == "avg":
        R = _mask(ref["p"].shape)
        for n, h, w, c in row.pos:
            R[n, h // 2, w // 2, c] = True
        outs["p"] = (R, R, ref["p"])
        fn = lambda q: dict(p=S.avgpool2_fwd(q["x"]))
    elif f == "smean":
        R = _mask(ref["y"].shape)
        for n, _, c in row.pos:
            R[n, c] = True
        outs["y"] = (R, R, S.f32(ref["y"]))
        fn = lambda q: dict(y=S.f32(S.spatial_mean_fwd(q["x"])))          # an exact sum, one division, one rounding
    elif f == "moments":
        g = p["g"]
        R = _mask(ref["out"].shape)
        for n, _, i in row.pos:
            grp = n if p["ps"] else 0
            R[grp, i] = True                                 # mean of g_i, then every product that holds g_i
            for j in range(g):
                R[grp, g + i * g + j] = R[grp, g + j * g + i] = True
        outs["out"] = (R, R, S.f32(ref["out"]))
        fn = lambda q: dict(out=S.f32(S.guide_moments(q["guide"], p["ps"])))
    elif f == "fc":
        R = _mask(ref["y"].shape)
        for pos in row.pos:
            if row.operand == "x":
                R[pos[0], :] = True
            elif row.operand == "w":
                R[:, pos[1]] = True
            else:
                R[:, pos[0]] = True
        outs["y"] = (R, R, ref["y"])
        fn = lambda q: dict(y=S.fc(q, p["relu"])["y"])
    elif f == "conv1d":
        L, k = p["l"], p["k"]
        pad = (k - 1) // 2
        R, A = _mask(ref["y"].shape), _mask(ref["y"].shape)
        for pos in row.pos:
            if row.operand == "x":
                R[pos[0], max(pos[1] - pad, 0):min(pos[1] + pad + 1, L), :] = True
            elif row.operand == "w":
                t, _, co = pos                               # output l reads input l + t - pad
                R[:, max(pad - t, 0):min(L + pad - t, L), co] = True
                A[:, :, co] = True
            else:
                R[:, :, pos[0]] = True
        outs["y"] = (R, A | R, ref["y"])
        fn = lambda q: dict(y=S.conv1d(q, k, p["relu"])["y"])
    else:
        raise KeyError(f)
    return dict(inputs=a, outs=outs, restate=fn, src=src)


def _maxpool1d_nan(x):
    """small_ops_cases._windows1 pads the odd tail with -inf; np.max over (NaN, -inf) is NaN as well, so it serves unchanged."""
    return S.maxpool1d_fwd(x)


def _norm(row):
    r = NP.BY_ID[row.src]
    st = NP.BF16S if row.prec == BF16S else NP.FP32S
    a = NP.make_inputs(r, "exact", st)
    pool = row.fam == "normpool"
    n, hw, c = r.n, r.hw, r.c
    R = _mask((n, hw, c))
    for pos in row.pos:
        if row.operand == "y":
            R[pos] = True
        elif row.operand in ("scale", "shift"):
            g, ch = pos                                      # statistics group: the sample (instance norm) or the whole batch
            R[(g if r.ps else slice(None)), :, ch] = True
        elif row.operand == "den":
            R[pos[0], :, pos[1]] = True
        elif row.operand == "gw":                            # [Ng, G, C]: every pixel whose guide value multiplies it
            R[(pos[0] if r.gps else slice(None)), :, pos[2]] = True
        else:
            raise KeyError(row.operand)
    outs = collections.OrderedDict()
    if pool:
        h, w = hw // r.w, r.w
        ref = NP.pool_reference(r, a, st)
        outs["z"] = (R, R, ref["z"])
        Rp = NP.norm_unit.window_view(R, n, h, w).any(3).reshape(n, hw // 4, c)
        outs["pooled"] = (Rp, Rp, ref["pooled"])

        def fn(q):
            z = NP.unit_reference(r, q)["z"]
            zs = z if st == NP.FP32S else NP.round_bf16(z)
            return dict(z=z, pooled=NP.norm_unit.pooled(zs, n, h, w))
    else:
        outs["z"] = (R, R, NP.unit_reference(r, a)["z"])
        fn = lambda q: dict(z=NP.unit_reference(r, q)["z"])
    return dict(inputs=a, outs=outs, restate=fn, src=r, storage=st)


_CONV64 = {}


def _conv64(key, x, w):
    """float64 SAME conv, kept per source row: the rows that poison neither x nor w share the clean one."""
    if key not in _CONV64:
        _CONV64[key] = _np64(tf_ops.conv_nd_same(_t64(x), _t64(w)))
    return _CONV64[key]


def _conv(row):
    case = CP.BY_ID[row.src]
    x, w, _, lsb = CP.make_inputs(case, "eighths")
    a = dict(x=_np64(x), w=_np64(w))
    y = _conv64(row.src, a["x"], a["w"])
    R, A = _conv_sets(y.shape, row, case.h, case.w)
    outs = collections.OrderedDict(y=(R, A, y))
    fn = lambda q: dict(y=_np64(tf_ops.conv_nd_same(_t64(q["x"]), _t64(q["w"]))))
    return dict(inputs=a, outs=outs, restate=fn, src=case, lsb=lsb)


def _aff(row):
    r = EP.AFF_BY_ID[row.src]
    x, w, scale, shift = EP.aff_inputs(r, "exact")
    if row.opt.get("bias_only"):
        scale = torch.ones_like(scale)
    a = dict(x=_np64(x), w=_np64(w), scale=_np64(scale), shift=_np64(shift))
    y = _conv64(row.src, a["x"], a["w"])
    z = np.maximum(y * a["scale"] + a["shift"], 0.0)
    if row.operand in ("x", "w"):
        R, A = _conv_sets(z.shape, row, r.h, r.w)
    else:
        R = _mask(z.shape)
        for (co,) in row.pos:
            R[..., co] = True
        A = R
    outs = collections.OrderedDict(z=(R, A, z))
    if row.opt["pool"]:
        outs["pooled"] = (_win_any(R), _win_any(A), S.maxpool2_fwd(z))

    def fn(q):
        yy = y if row.operand not in ("x", "w") else _np64(tf_ops.conv_nd_same(_t64(q["x"]), _t64(q["w"])))
        zz = _np64(torch.relu(_t64(yy) * _t64(q["scale"]) + _t64(q["shift"])))          # torch.relu(NaN) = NaN
        out = dict(z=zz)
        if row.opt["pool"]:
            out["pooled"] = _np64(torch.nn.functional.max_pool2d(_t64(zz).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        return out
    return dict(inputs=a, outs=outs, restate=fn, src=r)


def _deconv(row):
    r = DP.BY_ID[row.src]
    x, w, b, dup = DP.make_inputs(r, "exact", row.prec)
    a = dict(x=_np64(x), w=_np64(w), b=None if b is None else _np64(b))
    assert (b is not None) or row.operand != "b", row.id

    def up(q):
        pre = tf_ops.conv_transpose_ks(_t64(q["x"]), _t64(q["w"]), (r.kd, 2, 2), bias=None if q["b"] is None else _t64(q["b"]))
        return _np64(torch.relu(pre))
    clean = up(a)
    R = _mask(clean.shape)
    kd = r.kd
    for pos in row.pos:
        if row.operand == "x":
            n, d, h, ww, _ = pos                            # kernel == stride: input (d, h, w) owns a kd x 2 x 2 block of outputs
            R[n, kd * d:kd * d + kd, 2 * h:2 * h + 2, 2 * ww:2 * ww + 2, :] = True
        elif row.operand == "w":
            t, i, j, co, _ = pos
            R[:, t::kd, i::2, j::2, co] = True
        else:
            R[..., pos[0]] = True
    outs = collections.OrderedDict(up=(R, R, clean))
    return dict(inputs=a, outs=outs, restate=lambda q: dict(up=up(q)), src=r, dup=dup)


def conv3d_shape(row):
    """(N, D, H, W, Cin, Cout, kd, stride, live ranges or None, expected forward launches) of a conv3d row."""
    import test_gpu_ops3d as O3
    if row.prec == BF16:
        c = C3.BY_ID[row.src]
        return (c.n, c.d, c.h, c.w, c.cin, c.cout, c.kd, (1, 1, 1)), None, [c.fwd]
    if isinstance(row.src, tuple):                            # a shape of another path table, its forward launches beside it
        return row.src, None, list(row.opt["trace"])
    if row.opt.get("live"):
        n, dd, h, w, cin, cin_live, cout, cout_live, kd, stride = O3.LIVE_CASES[row.src]
        return (n, dd, h, w, cin, cout, kd, stride), (cin_live, cout_live), O3.EXACT_LIVE_TRACES[row.src][0]
    return O3.CASES[row.src], None, O3.EXACT_TRACES[row.src][0]


def _conv3d(row):
    (n, dd, h, w, cin, cout, kd, stride), live, trace = conv3d_shape(row)
    live_co = np.ones(cout, bool)
    if row.prec == BF16:
        x, wt, _, _ = C3.make_inputs(C3.BY_ID[row.src], "eighths")
        x, wt = x.double(), wt.double()
    else:
        import test_gpu_ops3d as O3
        x, wt, _, co, _ = O3.exact_inputs((n, dd, h, w, cin, cout, kd, stride), live)     # the operands of its exact_case
        if live is not None:
            live_co = co.numpy()
            assert all(any(lo <= p[-1] < hi for lo, hi in live[0]) for p in row.pos), row.id
    a = dict(x=_np64(x), w=_np64(wt))
    conv = lambda xx, ww: _np64(tf_ops.conv_nd_same(_t64(xx), _t64(ww), stride=stride))
    y = conv(a["x"], a["w"])
    # the sets from indicator masks: a convolution of zeros and ones has no NaN and no rounding in it
    ind = np.zeros_like(a[row.operand])
    for p in row.pos:
        ind[p] = 1.0
    if row.operand == "x":
        hit = conv(ind, np.ones((kd, 3, 3, cin, 1))) > 0                      # [N, Do, Ho, Wo, 1]
        R = np.broadcast_to(hit, y.shape) & live_co
        A = np.broadcast_to(hit, y.shape).copy()                               # padded outputs: 0 * NaN may or may not be formed
    else:
        R = conv(np.ones_like(a["x"]), ind) > 0                                # the taps that land inside the volume
        A = _mask(y.shape)
        for p in row.pos:
            A[..., p[-1]] = True
    outs = collections.OrderedDict(y=(R.copy(), A | R, y))
    return dict(inputs=a, outs=outs, restate=lambda q: dict(y=conv(q["x"], q["w"])), src=None, geom=(n, dd, h, w, cin, cout, kd, stride),
                live=live, trace=trace)


_BUILD = {"conv3d": _conv3d, "mp2": _small, "mp1": _small, "avg": _small, "smean": _small, "moments": _small, "fc": _small, "conv1d": _small,
          "norm": _norm, "normpool": _norm, "conv": _conv, "aff": _aff, "deconv": _deconv}
_CASES = {}


def case(row):
    """Everything of one row, computed once and shared: dict(row, inputs, outs = {name: (R, A, clean float64)}, restate, src)."""
    if row.id not in _CASES:
        c = _BUILD[row.fam](row)
        c["row"] = row
        _CASES[row.id] = c
    return _CASES[row.id]


def stored(a, prec):
    """float64 -> the value a tensor of the row's storage holds (bf16 storage: one rounding)."""
    return S.round_bf16(a) if prec == BF16S else S.f32(a)

