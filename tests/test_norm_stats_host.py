"""The batch statistics of the normalised conv units, restated in numpy (no GPU needed).

The conv epilogue writes fp32 row partials of sum y and sum y^2; norm_reduce_finalize_kernel (csrc/norm.hip) sums them in
fp64 in a fixed lane order -- through a first level of 64 row blocks (rows_reduce_l1_kernel, csrc/reduce.hip) when a group
has more than 256 rows -- rounds both sums to fp32 and takes var = E[y^2] - E[y]^2.  Each fp32 rounding costs about
2^-24 (var + mean^2) of the variance, so its relative error grows with (mean / std)^2.

Here: that arithmetic; the error growing with mean / std; the decision rule of the fix (a channel is refined from the
activations when mean^2 > T (var + eps)), with T derived from the restatement and pinned to the kernel's constant; and the
shifted second pass of norm_refine_kernel, exact on a constant channel.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_PIX = 128            # pixels per epilogue row partial in this model (a tile row of the tiled kernels)
BOUND = 1e-5             # relative rstd / variance error the GPU tests (tests/test_gpu_norm_stats.py) assert


def row_partials(y):
    """y [pixels, K] fp32 -> fp32 row partials [2][rows][K], each a sequential fp32 sum over ROW_PIX pixels."""
    y = np.asarray(y, np.float32)
    rows = y.shape[0] // ROW_PIX
    yr = y[:rows * ROW_PIX].reshape(rows, ROW_PIX, -1)
    s0 = np.zeros((rows, y.shape[1]), np.float32)
    s1 = np.zeros_like(s0)
    for j in range(ROW_PIX):
        v = yr[:, j]
        s0 = s0 + v
        s1 = s1 + v * v
    return np.stack((s0, s1))


def first_level(src):
    """rows_reduce_l1_kernel: [rows][K] -> [64][K]; block rb sums its chunk of rows in 4 strided fp64 lanes, then
    (lane0 + lane1 + lane2 + lane3) rounded to fp32."""
    rows = src.shape[0]
    rb_n = 64
    chunk = (rows + rb_n - 1) // rb_n
    out = np.zeros((rb_n, src.shape[1]), np.float32)
    for rb in range(rb_n):
        r0, r1 = rb * chunk, min(rb * chunk + chunk, rows)
        lanes = [np.zeros(src.shape[1]) for _ in range(4)]
        for rl in range(4):
            for r in range(r0 + rl, r1, 4):
                lanes[rl] = lanes[rl] + src[r].astype(np.float64)
        out[rb] = (((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]).astype(np.float32)
    return out


def final_sum(src):
    """norm_reduce_finalize_kernel's fp64 sum of [rows][K]: 16 row lanes (rows rl, rl + 16, ...), then lanes 0..15."""
    lanes = np.zeros((16, src.shape[1]))
    for r in range(src.shape[0]):
        lanes[r % 16] += src[r].astype(np.float64)
    t = np.zeros(src.shape[1])
    for j in range(16):
        t = t + lanes[j]
    return t


def finalize_one_pass(parts, count):
    """[2][rows][K] fp32 partials of one group -> (mean, var) as float64, the kernel's arithmetic."""
    src0, src1 = parts[0], parts[1]
    if src0.shape[0] > 256:
        src0, src1 = first_level(src0), first_level(src1)
    t0, t1 = final_sum(src0), final_sum(src1)
    m = t0.astype(np.float32).astype(np.float64) / count
    v = t1.astype(np.float32).astype(np.float64) / count - m * m
    return m, np.maximum(v, 0.0)


def refine_pass(y, p):
    """norm_refine_kernel's statistics: fp64 sums of d = y - p, d^2 with p = the one-pass fp32 mean (a sequential sum
    here; every partial sum is exact on a constant channel, so the kernel's order gives the same there)."""
    d = np.asarray(y, np.float32).astype(np.float64) - np.asarray(p, np.float32).astype(np.float64)
    n = float(y.shape[0])
    s0, s1 = d.sum(0), (d * d).sum(0)
    dm = s0 / n
    return np.asarray(p, np.float32).astype(np.float64) + dm, np.maximum(s1 / n - dm * dm, 0.0)


def rstd32(v, eps):
    return (np.float32(1.0) / np.sqrt(np.asarray(v, np.float64).astype(np.float32) + np.float32(eps))).astype(np.float64)


def errors(y, eps):
    """Relative variance and rstd errors of the one-pass statistics against float64 moments of the same fp32 y."""
    y64 = np.asarray(y, np.float32).astype(np.float64)
    m64, v64 = y64.mean(0), y64.var(0)
    _, v = finalize_one_pass(row_partials(y), float(y.shape[0]))
    ev = np.abs(v - v64) / v64
    er = np.abs(rstd32(v, eps) - 1.0 / np.sqrt(v64 + eps)) * np.sqrt(v64 + eps)
    return ev, er


def samples(kind, rng, pixels, k):
    """Unit-variance, zero-mean columns, continuous-valued as conv outputs are.  (Data of a few values only, such as
    +-1, makes the fp32 roundings of a row correlated; the kernels' sums have no bound better than (rows terms) x 2^-24
    there, and such channels are left to the threshold's margin.)"""
    if kind == "gauss":
        z = rng.standard_normal((pixels, k))
    else:
        z = (rng.random((pixels, k)) - 0.5) * np.sqrt(12.0)
    return (z - z.mean(0)) / z.std(0)


def kernel_threshold():
    src = open(os.path.join(ROOT, "boxsegliver_amd", "csrc", "norm.hip")).read()
    return float(re.search(r"constexpr double NORM_REFINE_T = ([0-9.]+);", src).group(1))


def test_first_level_runs_above_256_rows():
    rng = np.random.default_rng(1)
    y = (rng.standard_normal((300 * ROW_PIX, 3)) + 2.0).astype(np.float32)
    parts = row_partials(y)
    assert parts.shape[1] == 300
    m, v = finalize_one_pass(parts, float(y.shape[0]))
    y64 = y.astype(np.float64)
    assert np.allclose(m, y64.mean(0), rtol=1e-6) and np.allclose(v, y64.var(0), rtol=1e-5)


def test_one_pass_error_grows_with_mean_over_std():
    """The variance error of E[y^2] - E[y]^2 scales like (mean / std)^2: below the bound at small ratios, far above it at
    100 and 1000 (the regime the GPU tests put the kernels in)."""
    rng = np.random.default_rng(2)
    pixels, k = 300 * ROW_PIX, 16
    worst = {}
    for ratio in (0.0, 1.0, 10.0, 100.0, 1000.0):
        y = (ratio * 1.0371 + samples("gauss", rng, pixels, k)).astype(np.float32)     # no dyadic mean: no lucky roundings
        ev, _ = errors(y, 1e-3)
        worst[ratio] = ev.max()
    assert worst[0.0] < 1e-6 and worst[1.0] < 1e-6
    assert worst[100.0] > BOUND
    assert worst[1000.0] > 1e-3
    assert worst[10.0] < worst[100.0] < worst[1000.0]


def test_constant_channel_one_pass_versus_refined():
    """A constant, non-dyadic channel: the one-pass variance is not 0 (under eps 1e-6 that moves rstd by percents); the
    shifted second pass gives exactly 0 and the exact mean."""
    pixels = 300 * ROW_PIX
    cs = np.array([1.1, 0.3, 3.7, 1234.567, -2.9, 1e-3], np.float32)
    y = np.broadcast_to(cs, (pixels, cs.size)).copy()
    m, v = finalize_one_pass(row_partials(y), float(pixels))
    assert (v > 0).any()
    assert np.abs(rstd32(v, 1e-6) * np.sqrt(1e-6) - 1.0).max() > 1e-2
    m2, v2 = refine_pass(y, m.astype(np.float32))
    assert (v2 == 0.0).all()
    assert (m2.astype(np.float32) == cs).all()


def _worst_kept(T, rng):
    """Worst relative variance / rstd error over channels just inside m^2 <= T (var + eps)."""
    worst_v = worst_r = 0.0
    for eps in (1e-3, 1e-6):
        for var in (1e3 * eps, 1.0, 1e4):
            for rows in (96, 300):
                for kind in ("gauss", "uniform"):
                    k = 8
                    z = samples(kind, rng, rows * ROW_PIX, k)
                    mean = np.sqrt(T * (var + eps)) * (1.0 - 1e-3)
                    sign = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
                    y = (sign * mean + np.sqrt(var) * z).astype(np.float32)
                    y64 = y.astype(np.float64)
                    m64, v64 = y64.mean(0), y64.var(0)
                    kept = m64 * m64 <= T * (v64 + eps)
                    ev, er = errors(y, eps)
                    worst_v = max(worst_v, ev[kept].max(initial=0.0))
                    worst_r = max(worst_r, er[kept].max(initial=0.0))
    return worst_v, worst_r


def test_refine_threshold():
    """T = NORM_REFINE_T (csrc/norm.hip) is the largest power of 4 at which the channels the one-pass path keeps stay
    within a quarter of the GPU tests' 1e-5 bound in rstd and half of it in the variance (the margin covers the kernels'
    own summation orders, which differ from this model's sequential row sums).  At 4 T they no longer do."""
    T = kernel_threshold()
    rng = np.random.default_rng(3)
    wv, wr = _worst_kept(T, rng)
    assert wv <= BOUND / 2 and wr <= BOUND / 4, (T, wv, wr)
    wv4, wr4 = _worst_kept(4 * T, rng)
    assert wv4 > BOUND / 2 or wr4 > BOUND / 4, (4 * T, wv4, wr4)


def test_flag_rule_flags_the_gpu_test_ratios():
    """Every ratio >= 10 the GPU tests use (variance >= 1e3 eps) is flagged; ratios 0 and 1 are not."""
    T = kernel_threshold()
    for eps in (1e-3, 1e-6):
        v = 1e3 * eps
        for ratio, flagged in ((0.0, False), (1.0, False), (10.0, True), (100.0, True), (1000.0, True), (3000.0, True)):
            m = ratio * np.sqrt(v)
            assert (m * m > T * (v + eps)) == flagged, (eps, ratio)
