"""Case table and references of the 2-D LiTS batch kernel's edge suite (test_lits_batch_host.py on the CPU,
test_gpu_lits_batch_edges.py on the GPU).  CPU-only: numpy and oracle/lits_ops.py, no torch.

`unetk_lits_batch` (csrc/lits.hip, geometry in csrc/lits_geom.h) feeds every 2-D training run.  The suite holds it at the
coordinates the project trains at (a 512 x 512 store, outputs of 256 .. 512) and at the edges of its geometry.

Stores.  "big": 4 slices of 512 x 512; "small": 4 slices of 61 x 53.  A slice is a one-pixel checkerboard between the two ends
of the store's window plus integer noise of 1/32 of the window, so that a source coordinate that is off by eps moves the
normalised value by about eps per axis and a part of the pixels clips.  A label slice is the seven-colour checkerboard
((2 y + x + s) % 7) * 36 + ((7 y + 3 x) % 36), read with lab_scale = 36: every one-pixel shift, diagonal ones included, changes
the class, no reflection of a resized row maps the pattern onto itself (with five
colours the scale-2.5 rows did), and the remainder makes `/ lab_scale` a real division.  Label slice 3 of
the small store holds every value 0 .. 255 instead, for the rows that run lab_scale over 64, 1, 100 and 255.

References.
  R32  oracle.lits_ops.process_sample, the float32 restatement in TF's operation order, on the box clamped as the kernel
       clamps it (`clamp_box`; the identity on every row that is not a clamp row).  The kernel has to reproduce it.
  R64  `r64_sample`, written apart from R32: taps and weights from integer arithmetic, i0 = k (ch - 1) // (oh - 1), f = the
       remainder / (oh - 1), nearest = (2 k (ch - 1) + (oh - 1)) // (2 (oh - 1)); flips through the source index; lerp
       (rows of the crop first, then columns), clip and normalise in float64.  A mistake that the kernel shares with R32
       does not pass it.

The image bound against R32 (`image_bound`).  Kernel and R32 form the same float32 coordinate, taps and weights -- that is
what the suite pins -- and from there the kernel may only round differently: the compiler contracts `a + (b - a) * t` into one
fma where R32 rounds the product and the sum, and the division may round either way.  In raw slice units every intermediate
is below P = the power of two above the store's largest value (<= 2^16), so one float32 rounding is at most e = P * 2^-25
(half an ulp just below P).  With V the exact bilinear value:
  top and bottom lerp   tr - tl is exact (integers below 2^16); product and sum round: within 2 e of exact (fused: 1 e)
  vertical lerp         its inputs carry (1 - ly) * 2 e + ly * 2 e = 2 e; bot - top, the product and the sum round: + 3 e
  so each side is within 5 e of V and the two are within 10 e of each other; the clip is 1-Lipschitz
  v - lo                one rounding on each side: 12 e
  / (hi - lo)           fl(hi - lo) is the same number on both sides; the quotient is at most 1, so each side rounds by at
                        most 2^-25: one ulp of the normalised value together
  bound = 12 e / (hi - lo) + 2^-24.
The big store (P = 2^15, window about 30360) gives 4.5e-7, the small one (P = 2^11, window about 400) 1.9e-6.
test_lits_batch_host.py shows that the bound is honest -- R32 with its three lerps fused stays inside it on every row -- and
sharp enough: a coordinate taken as k * float32(1 / (oh - 1)) * (ch - 1), or an `f` taken from an fma, falls outside it on
every full-slice row.  The bound against R64 is the row's own max |R32 - R64|, computed where it is used, plus the above.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import lits_ops

F32 = np.float32
INT32_MAX = 2 ** 31 - 1
LB_SCALE = 36                    # of the group rows: seven classes fit a uint8 (LAB_SCALES has the rest)

Store = namedtuple("Store", "n hw ends seed")
STORES = {"big": Store(4, (512, 512), (640, 31000), 71), "small": Store(4, (61, 53), (1000, 1400), 72)}
EVERY_VALUE_SLICE = 3            # label slice of the small store that holds 0 .. 255

Row = namedtuple("Row", "chans seg box flip_lr flip_ud clip")
Group = namedtuple("Group", "name store out_hw boxes full")

# boxes are (off_y, off_x, ch, cw); `full`: the rows of these boxes are at workload coordinates (the wrong-coordinate variants
# must be separated on them).  Flips cycle through the four combinations with the row number, so box 3 of a group is flipped
# on both axes: the crops of 1 sit there.
GROUPS = [
    Group("ws256", "big", (256, 256), [(0, 0, 512, 512), (1, 3, 511, 509), (100, 20, 307, 461), (511, 511, 1, 1),
                                       (256, 256, 256, 256), (510, 510, 2, 2)], (0, 1, 2)),
    Group("up512x384", "big", (512, 384), [(129, 255, 383, 257)], (0,)),
    Group("floor64", "big", (64, 64), [(7, 9, 280, 280), (0, 0, 512, 512), (301, 99, 148, 148), (100, 200, 148, 280)], ()),
    Group("over22x24", "big", (22, 24), [(0, 0, 511, 511), (1, 1, 511, 511)], ()),
    Group("under8x15", "big", (8, 15), [(0, 0, 511, 511), (1, 1, 511, 511)], ()),
    Group("tie33", "small", (33, 33), [(0, 0, 49, 49), (12, 4, 49, 49), (20, 30, 17, 17), (59, 51, 2, 2)], ()),
    Group("tie9", "small", (9, 9), [(3, 5, 21, 21), (40, 32, 21, 21)], ()),
    Group("one1x1", "small", (1, 1), [(0, 0, 61, 53), (5, 7, 30, 11), (3, 2, 1, 40), (60, 52, 1, 1), (2, 3, 50, 1)], ()),
    Group("one1x13", "small", (1, 13), [(0, 0, 61, 53), (5, 7, 30, 11), (3, 2, 1, 40), (60, 52, 1, 1), (2, 3, 50, 1)], ()),
    Group("one31x1", "small", (31, 1), [(0, 0, 61, 53), (5, 7, 30, 11), (3, 2, 1, 40), (60, 52, 1, 1), (2, 3, 50, 1)], ()),
]
GROUP = {g.name: g for g in GROUPS}
CHANNELS = (1, 3, 8)

# what the table's rows exist for, per (crop, output) pair of one axis; test_lits_batch_host.py proves each from float32 and
# integer arithmetic alone
TIES = {(49, 33): 16, (17, 33): 16, (2, 33): 1, (21, 9): 4,            # coordinates that are exactly k + 0.5
        (11, 13): 2, (40, 13): 3, (30, 31): 1, (50, 31): 1}           # ... and the ones the scale-0 groups' other axis brings
FLOOR_BELOW = {(280, 64): 7, (512, 64): 4, (148, 64): 3,              # floorf(y * scale) == the exact floor - 1 (on no other pair)
               (511, 8): 1, (511, 15): 2}                             # ... the undershooting last coordinate among them
LAST_COORD = {(511, 22): +1, (511, 24): +1, (511, 8): -1, (511, 15): -1, (512, 64): -1}   # float32 last coordinate vs crop - 1

LAB_SCALES = (64, 1, 100, 255)
NOISE_SEEDS = (0, 123, 0xFFFFFFFF)

# the second loop trip: 2^24 + 4096 pixels, one sample, one channel, a 5 x 7 crop of the small store, flipped up-down
TRIP2_HW = (4097, 4096)
TRIP2_ROW = Row((1,), 2, (31, 17, 5, 7), 0, 1, (F32(1003), F32(1391)))

# clamp rows on the small store (61 x 53): negative offsets, offsets at and past the extent, extents of 0 and below, boxes
# reaching past the slice -- every requested number within a few rows of the slice
CLAMP_OUT_HW = (12, 10)
CLAMP_BOXES = [(-3, 4, 20, 20), (5, -2, 20, 20), (-1, -1, 70, 60), (61, 10, 5, 5), (10, 53, 5, 5), (64, 55, 3, 3),
               (20, 20, 0, 9), (20, 20, 9, 0), (20, 20, -2, -4), (50, 40, 15, 9), (40, 45, 9, 12), (58, 50, 6, 6),
               (-2, 50, 65, 4), (60, 52, 1, 1)]


# ------------------------------------------------------------------------------------------------- stores
@functools.lru_cache(maxsize=None)
def store(name):
    """(slices uint16 [n, h, w], label slices uint8 [n, h, w]) of a store, read-only."""
    st = STORES[name]
    rng = np.random.default_rng(st.seed)
    (h, w), (e0, e1) = st.hw, st.ends
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    amp = (e1 - e0) // 32
    im = np.empty((st.n, h, w), np.uint16)
    lb = np.empty((st.n, h, w), np.uint8)
    for s in range(st.n):
        v = np.where((yy + xx + s) & 1, e1, e0) + rng.integers(-amp, amp + 1, size=(h, w))
        im[s] = np.clip(v, 0, 65535).astype(np.uint16)
        lb[s] = ((2 * yy + xx + s) % 7) * LB_SCALE + (7 * yy + 3 * xx) % LB_SCALE
    if name == "small":
        lb[EVERY_VALUE_SLICE] = (yy * w + xx) % 256
    im.setflags(write=False)
    lb.setflags(write=False)
    return im, lb


def clamp_box(box, src_hw):
    """The crop box as lits_batch_kernel clamps it into the slice (the four min / max lines at the top of its loop)."""
    off_y, off_x = min(max(int(box[0]), 0), src_hw[0] - 1), min(max(int(box[1]), 0), src_hw[1] - 1)
    ch, cw = min(max(int(box[2]), 1), src_hw[0] - off_y), min(max(int(box[3]), 1), src_hw[1] - off_x)
    return off_y, off_x, ch, cw


# ------------------------------------------------------------------------------------------------- rows
@functools.lru_cache(maxsize=None)
def rows_of(name, channels):
    """The rows of a group at C = channels: every box at least once, the four flip combinations in turn, then four more rows
    on the first boxes: a padding slice (-1), a label slice of -1, a slice index equal to n_slices, and 2^31 - 1 as a slice and
    as the label slice."""
    g, st = GROUP[name], STORES[GROUP[name].store]
    centres = st.n - 1 if g.store == "small" else st.n            # small store: slice 3 carries the every-value label
    m = max(len(g.boxes), 4)
    rows = []
    for j in range(m + 4):
        centre = j % centres
        chans = [(centre + c - channels // 2) % centres for c in range(channels)]
        seg = centre
        k = j - m
        if k == 0:
            chans[0] = -1
        elif k == 1:
            seg = -1
        elif k == 2:
            chans[-1] = st.n
        elif k == 3:
            chans[(channels - 1) // 2] = INT32_MAX
            seg = INT32_MAX
        clip = (F32(st.ends[0] + 3 * j), F32(st.ends[1] - 5 * j))
        rows.append(Row(tuple(chans), seg, g.boxes[j % len(g.boxes)], j & 1, (j >> 1) & 1, clip))
    return tuple(rows)


def is_full(name, j):
    g = GROUP[name]
    return (j % len(g.boxes)) in g.full


def lab_scale_rows():
    """Rows over the every-value label slice of the small store: the whole slice one to one, and two resized crops."""
    e0, e1 = STORES["small"].ends
    clip = (F32(e0), F32(e1))
    seg = EVERY_VALUE_SLICE
    return (Row((0, 1, 2), seg, (0, 0, 61, 53), 0, 0, clip), Row((1, 2, 0), seg, (0, 0, 61, 53), 1, 1, clip),
            Row((2, -1, 1), seg, (3, 1, 40, 50), 1, 0, clip), Row((0, 0, 0), seg, (10, 2, 51, 30), 0, 1, clip))


LAB_SCALE_OUT_HW = (61, 53)


def clamp_rows(channels=3):
    e0, e1 = STORES["small"].ends
    rows = []
    for j, box in enumerate(CLAMP_BOXES):
        chans = tuple((j + c) % 3 for c in range(channels))
        rows.append(Row(chans, (j + 1) % 3, box, j & 1, (j >> 1) & 1, (F32(e0 - j), F32(e1 + 2 * j))))
    return tuple(rows)


def table(rows):
    """(int32 [N, C + 7] sample table, f32 [N, 2] clip) as unetk_lits_batch takes them."""
    tab = np.array([list(r.chans) + [r.seg] + list(r.box) + [r.flip_lr, r.flip_ud] for r in rows], dtype=np.int64)
    assert tab.min() >= -2 ** 31 and tab.max() <= INT32_MAX
    return tab.astype(np.int32), np.array([r.clip for r in rows], dtype=F32)


# ------------------------------------------------------------------------------------------------- R32
def r32_sample(store_name, row, out_hw, lab_scale=LB_SCALE, flips=True):
    """(image f32 [H, W, C], label int32 [H, W]): oracle.lits_ops.process_sample on the clamped box.  A slice index outside
    [0, n_slices) is a padding slice."""
    im, lb = store(store_name)
    n = im.shape[0]
    slices = [im[s] if 0 <= s < n else None for s in row.chans]
    seg = lb[row.seg] if 0 <= row.seg < n else None
    with np.errstate(invalid="ignore", divide="ignore"):          # a window with hi == lo divides 0 by 0
        return lits_ops.process_sample(slices, seg, list(clamp_box(row.box, im.shape[1:])), row.clip, out_hw, lab_scale,
                                       bool(row.flip_lr) and flips, bool(row.flip_ud) and flips)


def r32_batch(store_name, rows, out_hw, lab_scale=LB_SCALE):
    outs = [r32_sample(store_name, r, out_hw, lab_scale) for r in rows]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ------------------------------------------------------------------------------------------------- R64
def r64_axis(crop, out, flip):
    """(i0, i1, f float64, nearest) per output index of one axis, all from integer arithmetic."""
    k = np.arange(out, dtype=np.int64)
    if flip:
        k = out - 1 - k
    if out == 1:
        z = np.zeros(1, np.int64)
        return z, z, np.zeros(1, np.float64), z
    num, den = k * (crop - 1), out - 1
    i0 = num // den
    return i0, np.minimum(i0 + 1, crop - 1), (num - i0 * den) / float(den), (2 * num + den) // (2 * den)


def r64_sample(store_name, row, out_hw, lab_scale=LB_SCALE):
    """(image float64 [H, W, C], label int64 [H, W])."""
    im, lb = store(store_name)
    n = im.shape[0]
    off_y, off_x, ch, cw = clamp_box(row.box, im.shape[1:])
    y0, y1, fy, ny = r64_axis(ch, out_hw[0], row.flip_ud)
    x0, x1, fx, nx = r64_axis(cw, out_hw[1], row.flip_lr)
    lo, hi = float(row.clip[0]), float(row.clip[1])
    img = np.zeros(tuple(out_hw) + (len(row.chans),), np.float64)
    for c, s in enumerate(row.chans):
        if not 0 <= s < n:
            continue
        crop = im[s, off_y:off_y + ch, off_x:off_x + cw].astype(np.float64)
        horiz = crop[:, x0] * (1.0 - fx)[None, :] + crop[:, x1] * fx[None, :]                   # [ch, W]
        v = horiz[y0] * (1.0 - fy)[:, None] + horiz[y1] * fy[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            img[..., c] = (np.clip(v, lo, hi) - lo) / (hi - lo)
    lab = np.zeros(tuple(out_hw), np.int64)
    if 0 <= row.seg < n:
        lab = lb[row.seg][off_y + ny][:, off_x + nx].astype(np.int64) // lab_scale
    return img, lab


# ------------------------------------------------------------------------------------------------- the bound
def raw_rounding(store_name):
    """e: the largest error of one float32 rounding below P, the power of two above the store's largest value."""
    p = 1 << int(store(store_name)[0].max()).bit_length()
    assert p <= 1 << 16
    return p * 2.0 ** -25


def image_bound(store_name, clip):
    """|kernel - R32| per normalised pixel of a row with this window (the module docstring derives it)."""
    return 12.0 * raw_rounding(store_name) / float(F32(clip[1]) - F32(clip[0])) + 2.0 ** -24


def coord_error(crop, out):
    """How far the float32 coordinate k * fl((crop - 1) / (out - 1)) can lie from the exact one: the scale's rounding carried to
    the last index and the product's own rounding, each at most (crop - 1) * 2^-24."""
    return 0.0 if out == 1 else (crop - 1) * 2.0 ** -23


# ------------------------------------------------------------------------------------------------- float32 variants of R32
def coords32(crop, out, mode="tf"):
    """float32 source coordinates of one axis.  tf: k * fl((crop - 1) / (out - 1)), the kernel's and TF's form.
    recip: k * fl(1 / (out - 1)) * (crop - 1), a reciprocal multiply."""
    k = np.arange(out, dtype=F32)
    if out == 1:
        return np.zeros(1, F32)
    if mode == "recip":
        return ((k * (F32(1) / F32(out - 1))).astype(F32) * F32(crop - 1)).astype(F32)
    return (k * (F32(crop - 1) / F32(out - 1))).astype(F32)


def _taps32(crop, out, mode):
    p = coords32(crop, out, "recip" if mode == "recip" else "tf")
    i0 = np.minimum(np.floor(p).astype(np.int64), crop - 1)
    if mode == "fma_f":         # f = fma(k, scale, -i0): the product is never rounded on its own
        scale = np.float64(F32(crop - 1) / F32(out - 1)) if out > 1 else 0.0
        f = (np.arange(out, dtype=np.float64) * scale - i0).astype(F32)
    else:
        f = (p - i0.astype(F32)).astype(F32)
    return i0, np.minimum(i0 + 1, crop - 1), f


def _lerp32(a, b, t, fused):
    d = (b - a).astype(F32)
    if fused:                   # one rounding: the product of two float32 is exact in float64
        return (a.astype(np.float64) + d.astype(np.float64) * t.astype(np.float64)).astype(F32)
    return (a + (d * t).astype(F32)).astype(F32)


def variant_image(store_name, row, out_hw, mode):
    """The image of R32 restated here with one thing changed.  tf: nothing (equals R32 bit for bit); fused: the three lerps
    are fmas; recip / fma_f: the coordinate or the weight is formed differently (coords32, _taps32) -- what the kernel must
    not do."""
    im, _ = store(store_name)
    n = im.shape[0]
    off_y, off_x, ch, cw = clamp_box(row.box, im.shape[1:])
    y0, y1, ly = _taps32(ch, out_hw[0], mode)
    x0, x1, lx = _taps32(cw, out_hw[1], mode)
    ly, lx = ly[:, None], lx[None, :]
    lo, hi = F32(row.clip[0]), F32(row.clip[1])
    fused = mode == "fused"
    img = np.zeros(tuple(out_hw) + (len(row.chans),), F32)
    for c, s in enumerate(row.chans):
        if not 0 <= s < n:
            continue
        crop = im[s, off_y:off_y + ch, off_x:off_x + cw].astype(F32)
        top = _lerp32(crop[y0][:, x0], crop[y0][:, x1], lx, fused)
        bot = _lerp32(crop[y1][:, x0], crop[y1][:, x1], lx, fused)
        v = _lerp32(top, bot, ly, fused)
        with np.errstate(invalid="ignore", divide="ignore"):
            img[..., c] = ((np.clip(v, lo, hi) - lo) / (hi - lo)).astype(F32)
    if row.flip_lr:
        img = img[:, ::-1]
    if row.flip_ud:
        img = img[::-1]
    return np.ascontiguousarray(img)


def nearest32(crop, out, half_even=False):
    """Nearest source index of one axis from the float32 coordinate: roundf (half away from zero) as TF and the kernel, or
    rintf (half to even), the variant the tie rows must tell apart."""
    p = coords32(crop, out).astype(np.float64)
    r = np.rint(p) if half_even else np.floor(p + 0.5)
    return np.minimum(r.astype(np.int64), crop - 1)


def label_with(store_name, row, out_hw, half_even, lab_scale=LB_SCALE):
    """The label of a row through nearest32 (no flips applied)."""
    _, lb = store(store_name)
    off_y, off_x, ch, cw = clamp_box(row.box, lb.shape[1:])
    ny, nx = nearest32(ch, out_hw[0], half_even), nearest32(cw, out_hw[1], half_even)
    return lb[row.seg][off_y + ny][:, off_x + nx].astype(np.int64) // lab_scale


# ------------------------------------------------------------------------------------------------- noise
def u01(seed, counters):
    """`u01` of csrc/lits.hip in uint64 arithmetic (wrapping): the splitmix64 finaliser of the counter, its top 24 bits
    as a float64 in [0, 1)."""
    i = np.asarray(counters, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFF
    z = (i + np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(seed << 32 | seed)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def noise_field(seed, shape, noise_scale):
    """(2 u - 1) * noise_scale in float64 for an [N, H, W, C] image: element (i, c) draws counter i * C + c, i the pixel's
    index in the batch.  2 u - 1 is a multiple of 2^-23 inside [-1, 1): exact in float32 too."""
    count = int(np.prod(shape))
    u = u01(seed, np.arange(count, dtype=np.uint64)).reshape(shape)
    return (2.0 * u - 1.0) * float(F32(noise_scale))


def check_noise(noisy, clean, seed, noise_scale, real, what=""):
    """noisy == clean + (2 u - 1) * noise_scale to one float32 ulp of the sum (the product rounds, or is fused into the add,
    and the add rounds: two half ulps at most at the larger of the two magnitudes); exactly clean where `real` is False."""
    noisy64, clean64 = noisy.astype(np.float64), clean.astype(np.float64)
    want = noise_field(seed, noisy.shape, noise_scale)
    real = np.broadcast_to(real, noisy.shape)
    tol = np.spacing((np.abs(clean64) + np.abs(want)).astype(F32)).astype(np.float64)
    err = np.abs(noisy64 - (clean64 + want))
    bad = real & ~(err <= tol)
    if bad.any():
        first = np.argwhere(bad)[0]
        raise AssertionError("{}: {} of {} noise values off, first at {} (flat element {}): got {!r}, want {!r} + {!r}".format(
            what, int(bad.sum()), bad.size, first.tolist(), int(np.flatnonzero(bad.ravel())[0]), noisy[tuple(first)],
            clean[tuple(first)], want[tuple(first)]))
    assert np.array_equal(noisy[~real], clean[~real]), what + ": noise on a padding slice"
    return float(np.max(err[real] / tol[real])) if real.any() else 0.0
