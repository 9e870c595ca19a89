"""The table of tests/test_gpu_norm_paths.py (csrc/norm.hip: apply, backward, pool-fused, SE / dropout passes), the Python
restatement of the host dispatch it is checked against (tests/test_norm_paths_host.py, no GPU) and the inputs of both tiers.

What is restated is norm.hip's NormPlan: `geom` = stat_geom + launch_geom, `bwd_blocks`, `apply_grid`, `k_rows` = NormPlan::K,
`ws_bytes` = unetk_norm_bwd_ws_bytes (the segment-wise maximum of bwd_ws_layout), `plan` = norm_plan's geometry and grids of a
row.  tests/test_norm_plan_host.py holds the library's two queries to `ws_bytes` and to recorded values without a GPU.

A row names, by hand from the dispatch code of norm.hip, the template arguments of the kernels it must reach (`tmpl`: G, D, L as
GD_DISPATCH instantiates them) and the reducer launches behind unetk_rows_reduce_alias (`red`: "w" = rows_reduce_final_wide_kernel,
"l1" = rows_reduce_l1_kernel, "n" = rows_reduce_final_kernel); `xdy` marks the rows whose dy is compared bit for bit (the
statistics count Ps is a power of two and every intermediate of the dy expression is representable: asserted on the host).
"""
import collections

import numpy as np

from oracle import norm_unit
from unetk_rng import unit_mask_host

FP32S, BF16S = 0, 2
COL_BLOCKS, RR_DIRECT_ROWS, RR_WIDE_ROWS = 1024, 256, 1024
GROUPS, RGROUPS = 4, 2            # UNETK_NORM_GROUPS(_BF), UNETK_NORM_RGROUPS(_BF)
APPLY_CAP = 4096
SEED = 987654321

Row = collections.namedtuple(
    "Row", "id kind n hw c ps g den leaky keep affine gps gbare coff gstride zpad dzpad w pre prealign tmpl red xdy bf")


def _r(id, n, hw, c, ps, tmpl, red, g=0, den=False, leaky=0, keep=0.0, affine=False, gps=False, gbare=False, coff=0, gstride=None,
       zpad=0, dzpad=0, w=0, pre=0, prealign=True, xdy=False, bf=True, kind="unit"):
    gstride = (coff + c) if gstride is None else gstride
    return Row(id, kind, n, hw, c, int(ps), g, den, leaky, keep, affine, gps, gbare, coff, gstride, zpad, dzpad, w, pre, prealign,
               tmpl, tuple(red), xdy, bf)


PLAIN = "0,false,false"
ROWS = []

# ---- 1. thread map: cq_n = C / 4 quads x rpi = 256 / cq_n row lanes; C = 24, 96, 200, 516, 1000 leave idle threads.
#      HW = 8 (xdy: Ps = 8 or 16); batch norm = one launch group, instance norm = N
for _c in (4, 8, 24, 96, 200, 516, 1000, 1024):
    ROWS.append(_r("map_c%d_bn" % _c, 2, 8, _c, False, PLAIN, ["w"], xdy=True))
    ROWS.append(_r("map_c%d_in" % _c, 2, 8, _c, True, PLAIN, ["w", "w"], xdy=True))
for _c in (96, 516):               # K = 6 rows of LDS: the largest layout of the map
    ROWS.append(_r("map_c%d_g2d_bn" % _c, 2, 8, _c, False, "2,true,false", ["w", "w"], g=2, den=True, xdy=True))
    ROWS.append(_r("map_c%d_g2d_in" % _c, 2, 8, _c, True, "2,true,false", ["w", "w"], g=2, den=True, xdy=True))

# ---- 2. template switch: G = 0..4 x {plain, D, L, D+L, post}; HW = 37 is odd, C = 24 has idle threads, N = 3
for _g in range(5):
    ROWS.append(_r("t_g%d_plain" % _g, 3, 37, 24, _g % 2 == 0, "%d,false,false" % _g, ["w", "w"] if _g % 2 == 0 else ["w"], g=_g))
    ROWS.append(_r("t_g%d_d" % _g, 3, 37, 24, _g % 2 == 1, "%d,true,false" % _g, ["w", "w"], g=_g, den=True, gbare=(_g == 0)))
    if _g:
        ROWS.append(_r("t_g%d_l" % _g, 3, 37, 24, _g % 2 == 0, "%d,false,true" % _g, ["w", "w"] if _g % 2 == 0 else ["w"], g=_g,
                       leaky=2))
        ROWS.append(_r("t_g%d_dl" % _g, 3, 37, 24, _g % 2 == 1, "%d,true,true" % _g, ["w", "w"], g=_g, den=True, leaky=2))
        ROWS.append(_r("t_g%d_post" % _g, 3, 37, 24, _g % 2 == 0, "%d,true,true" % _g, ["w", "w"], g=_g, den=True, leaky=3))
ROWS += [
    _r("t_l_fixed02", 2, 16, 64, True, "1,false,true", ["w", "w"], g=1, leaky=1),                  # LGNet's fixed 0.2 slope: bound tier
    _r("t_dl_fixed02", 2, 16, 64, False, "2,true,true", ["w", "w"], g=2, den=True, leaky=1),
    _r("t_affine_only", 2, 16, 64, False, PLAIN, ["w"], affine=True, xdy=True),                    # a.plain: dy = scale dt
    _r("t_affine_only_in", 2, 16, 64, True, PLAIN, ["w", "w"], affine=True, xdy=True),
    _r("t_gps_in", 3, 16, 24, True, "2,false,false", ["w", "w"], g=2, gps=True, xdy=True),          # kb = 0
    _r("t_gps_d_bn", 3, 16, 24, False, "2,true,false", ["w", "w"], g=2, den=True, gps=True),        # kb = 2 + G, psum route
    _r("t_gps_l_in", 3, 16, 24, True, "1,false,true", ["w", "w"], g=1, leaky=2, gps=True, xdy=True),
    _r("t_gps_post", 3, 16, 24, True, "3,true,true", ["w", "w"], g=3, den=True, leaky=3, gps=True, xdy=True),   # post block groups = N
    _r("t_gbare_plain", 2, 16, 24, False, PLAIN, ["w"], gbare=True, xdy=True),                      # a bare post-shift: dgb = sum dt
    _r("t_gw_slice", 2, 16, 24, False, "2,false,false", ["w"], g=2, coff=24, gstride=72),
    _r("t_gw_slice_post", 2, 16, 24, True, "1,true,true", ["w", "w"], g=1, den=True, leaky=3, coff=8, gstride=40, xdy=True),
    _r("t_concat_slice", 2, 16, 24, False, PLAIN, ["w"], zpad=24, dzpad=40, xdy=True),             # z / dz strides > C, guards both sides
    _r("t_concat_slice_g1", 2, 16, 96, True, "1,false,false", ["w", "w"], g=1, zpad=8, dzpad=4, xdy=True),
    _r("t_drop_plain", 2, 64, 24, True, PLAIN, ["w", "w"], keep=0.5),                               # dropout leaves the unrolled loops
    _r("t_drop_d_g1", 3, 37, 24, False, "1,true,false", ["w", "w"], g=1, den=True, keep=0.25),
    _r("t_drop_l", 2, 37, 64, True, "2,false,true", ["w", "w"], g=2, leaky=2, keep=0.5),
    _r("t_drop_post", 2, 37, 64, False, "1,true,true", ["w", "w"], g=1, den=True, leaky=3, keep=0.25),
    # dy bit for bit in every template family, with and without dropout: HW = 16, so Ps = 16 (instance norm) or 32 (batch norm)
    _r("x_l_in", 2, 16, 24, True, "2,false,true", ["w", "w"], g=2, leaky=2, xdy=True),
    _r("x_l_bn", 2, 16, 24, False, "4,false,true", ["w"], g=4, leaky=2, xdy=True),
    _r("x_d_bn", 2, 16, 24, False, "1,true,false", ["w", "w"], g=1, den=True, xdy=True),
    _r("x_dl_in", 2, 16, 24, True, "1,true,true", ["w", "w"], g=1, den=True, leaky=2, xdy=True),
    _r("x_dl_bn", 2, 16, 96, False, "3,true,true", ["w", "w"], g=3, den=True, leaky=2, xdy=True),
    _r("x_post_in", 2, 16, 24, True, "2,true,true", ["w", "w"], g=2, den=True, leaky=3, xdy=True),
    _r("x_post_bn", 2, 16, 96, False, "4,true,true", ["w", "w"], g=4, den=True, leaky=3, xdy=True),
    _r("x_drop_plain", 2, 16, 24, True, PLAIN, ["w", "w"], keep=0.5, xdy=True),
    _r("x_drop_d", 2, 16, 24, False, "1,true,false", ["w", "w"], g=1, den=True, keep=0.25, xdy=True),
    _r("x_drop_l", 2, 16, 24, True, "1,false,true", ["w", "w"], g=1, leaky=2, keep=0.25, xdy=True),
    _r("x_drop_dl", 2, 16, 24, True, "2,true,true", ["w", "w"], g=2, den=True, leaky=2, keep=0.5, xdy=True),
    _r("x_drop_post", 2, 16, 24, False, "1,true,true", ["w", "w"], g=1, den=True, leaky=3, keep=0.5, xdy=True),
]

# ---- 3. row-group tails of the unrolled loops: C = 64, rpi = 16; apply passes 4 rpi = 64 rows per block pass, the reduction 32
for _p in (1, 15, 16, 63, 65, 31, 33):
    ROWS.append(_r("tail_p%d_bn" % _p, 1, _p, 64, False, PLAIN, ["w"], xdy=_p in (1, 16)))
    ROWS.append(_r("tail_p%d_in" % _p, 2, _p, 64, True, PLAIN, ["w", "w"], xdy=_p in (1, 16)))
for _p in (1, 41, 42, 167, 169, 83, 85):            # C = 24: rpi = 42 with idle threads
    ROWS.append(_r("tail24_p%d" % _p, 1, _p, 24, False, PLAIN, ["w"], xdy=_p == 1))

# ---- 4. grid caps: backward 1024 blocks (one launch group), max(2048 / L, 64) otherwise; apply 4096 and ceil(4096 / L).
#      A row group is rpi rows of C channels: 1024 elements where C / 4 divides 256, 516 at C = 516 (rpi = 1), the fewest there are
ROWS += [
    _r("cap_bwd_1024", 1, 16 * 1024, 64, False, PLAIN, ["w"]),                   # nblk = 1024 exactly
    _r("cap_bwd_1025", 1, 16 * 1025, 64, False, PLAIN, ["w"]),                   # 1025 row groups on 1024 blocks: grid stride
    _r("cap_bwd_l2", 2, 1025, 516, True, PLAIN, ["w", "w"], bf=False),           # L = 2: 1024 per group
    _r("cap_bwd_l40", 40, 65, 516, True, PLAIN, ["w", "w"], bf=False),           # L = 40: the 64-block floor, 65 row groups
    _r("cap_bwd_l40_at", 40, 64, 516, True, PLAIN, ["w", "w"], xdy=True, bf=False),
    _r("cap_apply_4096", 1, 4096, 516, False, PLAIN, ["w"]),                     # rpi = 1: 4096 row groups on 4096 blocks
    _r("cap_apply_4097", 1, 4097, 516, False, PLAIN, ["w"], bf=False),
    _r("cap_apply_l3", 3, 1367, 516, True, PLAIN, ["w", "w"], bf=False),         # ceil(4096 / 3) = 1366 blocks, 1367 row groups
]

# ---- 5. reducer routes: nblk = 256, 257, 1024 (above); pre_partials with 1, 256, 257, 1024, 1025 rows per launch group
ROWS += [
    _r("red_nblk256", 1, 256, 1024, False, PLAIN, ["w"], xdy=True),
    _r("red_nblk257", 1, 257, 1024, False, PLAIN, ["w"]),
    _r("red_d_bn_n3", 3, 37, 24, False, "0,true,false", ["w", "w"], den=True, gbare=True),      # second level into psum
    _r("red_simple_l1", 1, 64, 64, False, PLAIN, ["w"], xdy=True),                               # dbeta / dgamma by the only launch
    _r("red_simple_l3", 3, 64, 64, True, PLAIN, ["w", "w"], xdy=True),                           # ... by the second-level launch
    _r("pre_1", 1, 64, 64, False, PLAIN, ["w"], pre=1, xdy=True),
    _r("pre_256", 1, 512, 64, False, PLAIN, ["w"], pre=256, xdy=True),
    _r("pre_257", 1, 514, 64, False, PLAIN, ["w"], pre=257),
    _r("pre_1024", 1, 1024, 64, False, PLAIN, ["w"], pre=1024, xdy=True),
    _r("pre_1025", 1, 1025, 64, False, PLAIN, ["l1", "w"], pre=1025),
    _r("pre_in_l3k5", 3, 40, 64, True, PLAIN, ["w", "w"], pre=15),                               # L k rows under instance norm
    _r("pre_in_l2k1025", 2, 1025, 24, True, PLAIN, ["l1", "w", "w"], pre=2050),
    _r("pre_unaligned_257", 1, 514, 64, False, PLAIN, ["l1", "n"], pre=257, prealign=False),     # 4-byte aligned partials: narrow route
    _r("pre_unaligned_8", 1, 64, 24, False, PLAIN, ["n"], pre=8, prealign=False, xdy=True),
]

# ---- 6. pool-fused: W (and H = HW / W) even; windows per launch group Q = HW / 4 (x N under batch norm)
ROWS += [
    _r("pool_2x2", 1, 4, 64, False, "", ["w"], w=2, kind="pool", xdy=True),
    _r("pool_2x6_bn_n3", 3, 12, 24, False, "", ["w"], w=6, kind="pool"),                         # img = q / per_img
    _r("pool_6x2_in_n3", 3, 12, 24, True, "", ["w", "w"], w=2, kind="pool"),                     # img = n
    _r("pool_8x8_dskip", 2, 64, 64, False, "", ["w"], w=8, dzpad=64, kind="pool", xdy=True),     # dskip = a slice of the concat gradient
    _r("pool_8x8_in_c8", 2, 64, 8, True, "", ["w", "w"], w=8, dzpad=8, kind="pool", xdy=True),
    _r("pool_cap_1024", 1, 4096, 516, False, "", ["w"], w=64, kind="pool", bf=False),            # 1024 windows = the reduce pass's cap
    _r("pool_cap_1025", 1, 4100, 516, False, "", ["w"], w=2, kind="pool"),                       # one window over it
    _r("pool_cap_in_l2", 2, 4100, 516, True, "", ["w", "w"], w=2, kind="pool", bf=False),
    # the 4096-block cap of the two pool APPLY passes: 4096 and 4097 windows of four pixels, 8.5 M elements per tensor
    _r("pool_apply_cap_4096", 1, 4 * 4096, 516, False, "", ["w"], w=128, kind="pool", bf=False),
    _r("pool_apply_cap_4097", 1, 4 * 4097, 516, False, "", ["w"], w=2, kind="pool", bf=False),
]

# ---- 7. SE / dropout side passes: one launch group per sample
for _n in (1, 5):
    for _hw in (1, 3):
        for _c in (24, 1024):
            ROWS.append(_r("se_n%d_p%d_c%d" % (_n, _hw, _c), _n, _hw, _c, (_n + _hw) % 2 == 0, "", [], keep=0.5, kind="se"))
ROWS += [
    _r("se_cap_n1", 1, 4097, 516, True, "", [], keep=0.25, kind="se", bf=False),                # 4096 blocks, 4097 row groups
    _r("se_cap_n5", 5, 821, 516, False, "", [], keep=0.5, kind="se", bf=False),                 # ceil(4096 / 5) = 820 blocks
    _r("se_c24_p100", 2, 100, 24, False, "", [], keep=0.5, kind="se"),                          # several passes of 42 row lanes
]
del _c, _g, _p, _n, _hw

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


# ------------------------------------------------------------------ the host dispatch of norm.hip, restated
def colmap(c):
    cq_n = c // 4
    return cq_n, 256 // cq_n


def geom(row, density):
    """NormGeom: (Ns, Ps, L, P, sst)."""
    ns = row.n if row.ps else 1
    ps = row.hw if row.ps else row.n * row.hw
    L = row.n if (row.ps or density) else 1
    p = row.hw if L > 1 else row.n * row.hw
    return ns, ps, L, p, (row.c if row.ps else 0)


def _cd(a, b):
    return -(-a // b)


def bwd_blocks(p, rpi, L):
    cap = max(2048 // L, 64) if L > 1 else COL_BLOCKS
    return min(_cd(p, rpi), cap)


def apply_grid(p, rpi, L):
    return min(_cd(p, rpi), _cd(APPLY_CAP, L) if L > 1 else APPLY_CAP)


def k_rows(row):
    return 2 + row.g + (2 if row.den else (1 if row.leaky else 0)) + (1 if row.leaky == 3 else 0)


def tmp_floats(k, rows, c):
    return k * 64 * c if rows > RR_DIRECT_ROWS else 0


def ws_bytes(row):
    """unetk_norm_bwd_ws_bytes restated."""
    _, rpi = colmap(row.c)
    k = 5 + row.g
    _, _, Ld, pd, _ = geom(row, True)
    _, _, L1, p1, _ = geom(row, False)
    f = k * max(Ld * bwd_blocks(pd, rpi, Ld), L1 * bwd_blocks(p1, rpi, L1)) * row.c
    f += k * Ld * row.c + k * row.c
    f += tmp_floats(k * Ld, RR_DIRECT_ROWS + 1, row.c) + tmp_floats(k, Ld, row.c)
    return 4 * f


def reduce_route(rows, aligned=True):
    """unetk_rows_reduce_alias: the launches for `rows` source rows (C % 4 == 0 throughout)."""
    out = []
    if rows > (RR_WIDE_ROWS if aligned else RR_DIRECT_ROWS):
        out.append("l1")
        out.append("w" if aligned else "n")      # `wide` was decided on the caller's pointer, before the first level
        return out
    return ["w" if aligned else "n"]


def plan(row):
    """Everything the host decides for a row: dict(cq_n, rpi, idle, L, P, Ps, nblk, gx, red, K, lds)."""
    cq_n, rpi = colmap(row.c)
    ns, ps, L, p, sst = geom(row, row.den or row.kind == "se")
    q = p // 4 if row.kind == "pool" else p
    nblk = bwd_blocks(q, rpi, L)
    gx = apply_grid(q, rpi, L)
    if row.pre:
        red = reduce_route(row.pre // L, row.prealign)
    else:
        red = reduce_route(nblk)
    if L > 1:
        red = red + reduce_route(L)
    k = 2 if row.kind == "pool" else k_rows(row)
    return dict(cq_n=cq_n, rpi=rpi, idle=256 - cq_n * rpi, L=L, P=p, Ps=ps, Ns=ns, Q=q, nblk=nblk, gx=gx, red=red, K=k,
                lds=k * rpi * row.c * 4, sst=sst)


RED_NAME = {"w": "rows_reduce_final_wide_kernel", "l1": "rows_reduce_l1_kernel", "n": "rows_reduce_final_kernel"}


def tname(storage):
    return "unsignedshort" if storage == BF16S else "float"


def expected_apply(row, storage):
    if row.kind == "pool":
        return ["norm_apply_relu_pool_kernel<%s>" % tname(storage)]
    return ["norm_apply_relu_kernel<%s,%s>" % (row.tmpl, tname(storage))]


def expected_bwd(row, storage):
    """The backward's launches in order, from the row's hand-written tmpl / red."""
    t = tname(storage)
    red = [RED_NAME[r] for r in row.red]
    if row.kind == "pool":
        return ["norm_bwd_reduce_pool_kernel<%s>" % t] + red + ["norm_bwd_apply_pool_kernel<%s>" % t]
    out = [] if row.pre else ["norm_bwd_reduce_kernel<%s,%s,%s>" % (row.tmpl, t, "true" if row.leaky == 3 else "false")]
    out += red
    simple = row.g == 0 and not row.den and not row.leaky and not row.gbare
    if not simple:
        out.append("norm_bwd_params_kernel")
    if row.gps:
        out.append("norm_bwd_guide_ps_kernel")
    if row.leaky == 3:
        out.append("norm_bwd_post_block_kernel")
    return out + ["norm_bwd_apply_kernel<%s,%s>" % (row.tmpl, t)]


# ------------------------------------------------------------------ inputs
def round_bf16(a):
    """float64 / float32 array -> the bf16 value it rounds to (RNE), as float64."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def is_f32(a):
    a = np.asarray(a, np.float64)
    return bool(np.all(a.astype(np.float32).astype(np.float64) == a))


def sum_exact(terms, axes):
    """Sums of `terms` over `axes` are exact in fp32 in ANY order: all terms are multiples of one power of two 2^-k and the
    sum of their magnitudes stays under 2^24 of that unit."""
    t = np.asarray(terms, np.float64)
    for k in range(0, 16):
        if np.all(np.rint(t * 2.0 ** k) == t * 2.0 ** k):
            return bool(np.abs(t).sum(axes).max() * 2.0 ** k < 2.0 ** 24)
    return False


def make_inputs(row, kind, storage):
    """float32-representable float64 arrays of one row: `exact` (the exact tier's table of values) or `gauss`."""
    rng = np.random.default_rng(1000 + sum(ord(ch) for ch in row.id) * 7 + (0 if kind == "exact" else 1))
    n, hw, c, g = row.n, row.hw, row.c, row.g
    ns = n if row.ps else 1
    ng = n if row.gps else 1
    a = {}
    pick = lambda vals, shape: np.asarray(vals, np.float64)[rng.integers(0, len(vals), shape)]
    if kind == "exact":
        y = rng.integers(-4, 5, (n, hw, c)).astype(np.float64)
        if n * hw >= 8:
            y *= (rng.random((n, hw, 1)) >= 0.125)                       # one pixel in eight is zero
        mean = rng.integers(-2, 3, (ns, c)).astype(np.float64)
        rstd = pick([0.5, 1.0, 2.0], (ns, c))
        gamma = pick([-1.0, -0.5, 0.5, 1.0, 2.0], (c,))
        beta = rng.integers(-8, 9, (c,)) / 8.0
        gamma[3 % c] = 0.0                                                # channel 3: scale = shift = 0 -> u == 0 ties at the ReLU
        beta[3 % c] = 0.0
        scale = gamma[None] * rstd
        shift = beta[None] - mean * scale
        dz = rng.integers(-2, 3, (n, hw, c)).astype(np.float64)
        a["den"] = pick([0.5, 1.0, 2.0], (n, c))
        a["guide"] = rng.integers(0, 4, (n, hw, max(g, 1))).astype(np.float64)[..., :g]
        a["gw"] = rng.integers(-8, 9, (ng, g, c)) / 8.0
        bias = rng.integers(-8, 9, (ng, c)) / 8.0
        if row.kind == "pool":
            # equal windows and a maximum at each position come from y itself: window k of a plane copies one pixel to all four
            # places (k % 5 == 0) or lifts place (k % 5) - 1; channel 5 % c ties only after rounding to bf16 (64 + y / 4)
            h, w = hw // row.w, row.w
            win = norm_unit.window_view(y, n, h, w)
            kidx = np.arange(win.shape[1] * win.shape[2]).reshape(win.shape[1], win.shape[2])
            for pos in range(5):
                sel = (kidx % 5) == pos
                if pos == 0:
                    win[:, sel] = win[:, sel][:, :, :1]
                else:
                    win[:, sel, pos - 1] = 4.0
            y = norm_unit.window_unview(win, n, h, w)
            ch = 5 % c
            scale[:, ch], shift[:, ch] = 0.25, 64.0
            rstd[:, ch] = 0.5
    else:
        y = rng.standard_normal((n, hw, c)) * 2 + 0.5
        if storage == BF16S:
            y = round_bf16(y)
        ax = (1,) if row.ps else (0, 1)
        eps = 1e-6 if row.ps else 1e-3
        mean = y.mean(ax).reshape(ns, c)
        var = y.var(ax).reshape(ns, c)
        if hw * (1 if row.ps else n) == 1:
            var = var + 1.0                                               # one pixel: keep rstd finite and ordinary
        rstd = 1.0 / np.sqrt(var + eps)
        gamma = (rng.random(c) + 0.5) * np.where(rng.random(c) < 0.2, -1.0, 1.0)
        beta = rng.standard_normal(c) * 0.3
        f32 = lambda v: v.astype(np.float32).astype(np.float64)
        mean, rstd = f32(mean), f32(rstd)
        scale = f32(gamma[None] * rstd)
        shift = f32(beta[None] - mean * scale)
        dz = rng.standard_normal((n, hw, c))
        a["den"] = f32(rng.random((n, c)) + 0.5)
        a["guide"] = f32(rng.random((n, hw, g)))
        a["gw"] = f32(rng.standard_normal((ng, g, c)) * 0.5)
        bias = f32(rng.standard_normal((ng, c)) * 0.2)
        dz = round_bf16(dz) if storage == BF16S else f32(dz)
        y = y if storage == BF16S else f32(y)
    a.update(y=y, dz=dz, mean=mean, rstd=rstd, scale=scale, shift=shift)
    if not row.den:
        a["den"] = None
    if not g:
        a["guide"] = a["gw"] = None
    a["gb"] = None
    if g or row.gbare:
        a["gb"] = bias
        if row.leaky == 3:
            if kind == "exact":
                ps = rng.integers(-8, 9, (ng, c)) / 8.0
            else:
                ps = (rng.standard_normal((ng, c)) * 0.2).astype(np.float32).astype(np.float64)
            ap = rng.integers(0, 2, (ng, c)).astype(np.float64)
            a["gb"] = np.stack([bias, ap, 1.0 - ap, ps], 1)
    a["alpha"] = {0: 0.0, 1: 0.2, 2: 0.25 if kind == "exact" else 0.3, 3: 0.0}[row.leaky]
    a["mask"] = unit_mask_host(SEED, (n, hw, c), row.keep).astype(np.float64) if row.keep else None
    if row.kind == "pool":
        q = hw // 4
        if kind == "exact":
            a["dp"] = rng.integers(-2, 3, (n, q, c)).astype(np.float64)
        else:
            dp = rng.standard_normal((n, q, c))
            a["dp"] = round_bf16(dp) if storage == BF16S else dp.astype(np.float32).astype(np.float64)
    if row.kind == "se":
        gs = (ns, c)
        if kind == "exact":
            a["A"] = rng.integers(-8, 9, (n, c)) / 8.0
            a["k1"], a["k2"] = rng.integers(-8, 9, gs) / 8.0, rng.integers(-8, 9, gs) / 8.0
        else:
            f32 = lambda v: v.astype(np.float32).astype(np.float64)
            a["A"] = f32(rng.standard_normal((n, c)) * 0.1)
            a["k1"], a["k2"] = f32(rng.standard_normal(gs) * 0.05), f32(rng.standard_normal(gs) * 0.05)
    return a


def unit_reference(row, a, dz=None):
    return norm_unit.unit(a["y"], a["dz"] if dz is None else dz, a["mean"], a["rstd"], a["scale"], a["shift"], bool(row.ps),
                          den=a["den"], guide=a["guide"], gw=a["gw"], gb=a["gb"], mask=a["mask"], leaky=row.leaky,
                          alpha=a["alpha"], affine_only=row.affine, per_sample_guide=row.gps)


def pre_partials(row, ref):
    """[2][pre_rows][C] as the producing conv's tiles would leave them: each launch group's pixels cut into pre_rows / L runs."""
    _, _, L, p, _ = geom(row, False)
    k = row.pre // L
    du = ref["du"].reshape(L, p, row.c)
    dux = (ref["du"] * ref["xhat"]).reshape(L, p, row.c)
    cuts = [(i * p) // k for i in range(k + 1)]
    part = np.zeros((2, L, k, row.c))
    for i in range(k):
        part[0, :, i] = du[:, cuts[i]:cuts[i + 1]].sum(1)
        part[1, :, i] = dux[:, cuts[i]:cuts[i + 1]].sum(1)
    return part.reshape(2, row.pre, row.c)


def exact_tier_is_bitwise(row):
    """The fixed 0.2 slope is no binary fraction: those rows compare at the bounds in both tiers."""
    return row.leaky != 1


def pool_reference(row, a, storage):
    """The fused pool pair: z = relu(t) as stored, its 2 x 2 maxima, dz = rnd(dskip + route(dp)) and the unit's backward on it."""
    rnd = round_bf16 if storage == BF16S else None
    n, h, w = row.n, row.hw // row.w, row.w
    fwd = unit_reference(row, a)
    z_st = fwd["z"] if rnd is None else rnd(fwd["z"])
    dz = norm_unit.pool_route(z_st, a["dz"], a["dp"], n, h, w, rnd)
    out = unit_reference(row, a, dz=dz)
    out["z"], out["pooled"], out["dz"] = fwd["z"], norm_unit.pooled(z_st, n, h, w), dz
    return out
