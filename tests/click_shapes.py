"""Label slices and click draws of the reference-pinned click records (tests/golden/ref_clicks.json): no GPU code, no RNG.

A mask is a union of ellipses (cy, cx, ry, rx) and rectangles (y0, x0, y1, x1; both corners inside) given as integers;
ellipse membership is (y - cy)^2 rx^2 + (x - cx)^2 ry^2 <= ry^2 rx^2 in int64, so tests/golden/make_click_fixtures.py (which
runs the reference on the masks) and the tests rebuild bit-identical label slices.  The fixture stores the popcount and the
sum of the flat indices of every mask; `build` is checked against both before a mask is used.

SHAPES lists the records' inputs.  Each shape is one crop of one slice and two click_tab rows (data/lits_inter.draw_click_tab
documents the columns): four foreground clicks with four background clicks of strategy 1, and the same with strategy 3.
What each shape is there for is said in DESIGN.md 7.3.5 and asserted in test_ref_clicks_host.py."""
import numpy as np

REF_CLICKS = (3, 10, 40, 5)                   # margin, step, band, max_clicks of the reference (gen_kernel :548-560)
SMALL_CLICKS = (1, 3, 5, 5)
CAP255_CLICKS = (3, 10, 251, 5)               # margin + band + 1 = 255: the largest cap the ABI admits
LAST = 0xFFFFFFFF
WAVES = 16                                    # of clk_select_kernel
TRIP = 512                                    # pixels a wave takes per loop trip (64 lanes x CLK_U)


def rank_draw(rank, count):
    """A 32-bit draw r with (r * count) >> 32 == rank."""
    r = ((rank << 32) + count - 1) // count
    assert (r * count) >> 32 == rank and r < 1 << 32
    return r


def chunk_of(total):
    """Pixels of a wave of clk_select_kernel: ceil(ceil(total / 16) / 64) * 64."""
    return ((total + WAVES - 1) // WAVES + 63) // 64 * 64


def build(shape, ellipses=(), rects=()):
    """uint8 [H, W] in {0, 1}."""
    h, w = shape
    yy = np.arange(h, dtype=np.int64)[:, None]
    xx = np.arange(w, dtype=np.int64)[None, :]
    m = np.zeros((h, w), bool)
    for cy, cx, ry, rx in ellipses:
        m |= (yy - cy) ** 2 * (rx * rx) + (xx - cx) ** 2 * (ry * ry) <= ry * ry * rx * rx
    for y0, x0, y1, x1 in rects:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m.astype(np.uint8)


def checksum(mask):
    """(popcount, sum of the flat indices of the object pixels)."""
    idx = np.flatnonzero(mask)
    return int(len(idx)), int(idx.astype(np.int64).sum())


# name -> (slice shape, ellipses, rects)
MASKS = {
    # an ellipse whose band reaches all four crop borders, a blob in the last rows
    "m100": ((100, 104), [(44, 54, 24, 34), (90, 20, 7, 12)], []),
    # everything on the right: the left 150 columns are farther than 128 from any object column and the top-left corner
    # farther than 255 from any object pixel; the rectangle's right edge is column 257 of the crop, the last rows hold object
    "m140": ((140, 333), [(65, 266, 30, 40), (11, 296, 4, 9)], [(111, 216, 134, 273)]),
    "m140_none": ((140, 333), [], []),
    "m140_all": ((140, 333), [], [(0, 0, 139, 332)]),
    "m12": ((12, 1024), [(6, 500, 5, 300)], [(0, 900, 11, 960)]),
    "m9": ((1024, 9), [(500, 4, 300, 3)], [(0, 0, 55, 8), (1000, 0, 1023, 8)]),
    "m1024": ((1024, 1024), [(512, 400, 300, 200), (900, 900, 30, 50), (40, 200, 30, 60), (990, 600, 25, 80)], []),
    # three 2 x 2 objects in waves 0, 7 and 15: the erosion leaves nothing ("small"), the mean is summed across the waves;
    # every background band ends one pixel inside the crop
    "m1024_tiny": ((1024, 1024), [], [(44, 60, 45, 61), (500, 700, 501, 701), (978, 960, 979, 961)]),
}

# 0 is rank_draw(0, count) and LAST gives rank count - 1 for every count below 2^32: the first and the last candidate alive in
# row-major order, whatever the count; the other two land mid-way
_FG = [0, LAST, 1 << 31, 12345]
_BG = [LAST, 0, 3 << 30, 1 << 31]


def _rows(n_fg=4, n_bg=4, fg=_FG, bg=_BG):
    return [[n_fg, n_bg, strategy, 0] + list(fg) + list(bg) for strategy in (1, 3)]


# id, mask, centre (cy, cx), crop (ch, cw), parameters, click_tab rows
SHAPES = [
    ("two_trips", "m100", (90, 95), (96, 100), REF_CLICKS, _rows()),
    ("wide", "m140", (70, 166), (130, 300), REF_CLICKS, _rows()),
    ("wide_cap255", "m140", (70, 166), (130, 300), CAP255_CLICKS, _rows()),
    ("wide_small", "m140", (70, 166), (130, 300), SMALL_CLICKS, _rows()),
    ("row_limit", "m12", (6, 512), (12, 1024), REF_CLICKS, _rows()),
    ("col_limit", "m9", (512, 4), (1024, 9), REF_CLICKS, _rows()),
    ("full", "m1024", (512, 512), (1024, 1024), REF_CLICKS, _rows()),
    ("full_tiny", "m1024_tiny", (512, 512), (1024, 1024), REF_CLICKS, _rows()),
    ("wide_none", "m140_none", (70, 166), (130, 300), REF_CLICKS, [_rows(n_bg=0)[0], _rows(n_bg=1)[1]]),
    ("wide_all", "m140_all", (70, 166), (130, 300), REF_CLICKS, _rows()),
]


def launches():
    """The records grouped as the device test launches them: [(slice shape, parameters, [mask names], [(id, slice index in the
    launch's store, centre, crop, click_tab row)])], rows of one slice shape and one parameter set together."""
    out = {}
    for sid, mask, centre, crop, params, rows in SHAPES:
        key = (MASKS[mask][0], params)
        names, recs = out.setdefault(key, ([], []))
        if mask not in names:
            names.append(mask)
        for row in rows:
            recs.append((sid, names.index(mask), centre, crop, row))
    return [(shape, params, names, recs) for (shape, params), (names, recs) in out.items()]
