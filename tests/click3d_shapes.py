"""Label volumes and click draws of the reference-pinned 3-D click records (tests/golden/ref_clicks3d.json): no GPU code, no RNG.

A volume is a list of slices, each a union of click_shapes' integer ellipses and rectangles, so tests/golden/
make_click3d_fixtures.py (which runs the reference on the volumes) and the tests rebuild bit-identical labels.  The fixture
stores the popcount and the sum of the flat indices of every volume; `build` is checked against both before a volume is used.

RECORDS lists the records' inputs: one case (the volume), one sample (centre, patch depth D, crop) and two click_tab rows
(data/lits_inter.draw_click_tab documents the columns): four clicks of each kind asked, the background once with strategy 1
and once with strategy 3.  What each record is there for is said in DESIGN.md 7.3.6 and asserted in
test_lits3d_clicks_host.py; draws that are neither 0 nor LAST were chosen with `click_shapes.rank_draw` so that the pick lands
where the record needs it."""
import numpy as np

import click_shapes as cs

REF_CLICKS, SMALL_CLICKS, LAST = cs.REF_CLICKS, cs.SMALL_CLICKS, cs.LAST
WAVES, TRIP = cs.WAVES, cs.TRIP               # of clk3_select_kernel: 16 waves share a slice, 512 pixels per loop trip


def chunk_of(area):
    """Pixels of one slice that a wave of clk3_select_kernel takes: ceil(ceil(area / 16) / 64) * 64."""
    return cs.chunk_of(area)


def build(name):
    """uint8 [depth, H, W] in {0, 1}."""
    shape, slices = VOLUMES[name]
    return np.stack([cs.build(shape, ellipses, rects) for ellipses, rects in slices])


def checksum(vol):
    """(popcount, sum of the flat indices of the object voxels)."""
    idx = np.flatnonzero(vol)
    return int(len(idx)), int(idx.astype(np.int64).sum())


_E = ([], [])
# name -> (slice shape, [(ellipses, rects) per slice])
VOLUMES = {
    # an object that grows and shrinks through the slices, a second blob on two of them, empty first and last slices
    "v100": ((100, 104), [_E, ([(44, 54, 14, 20)], []), ([(44, 54, 20, 28), (88, 18, 7, 10)], []),
                          ([(44, 54, 24, 34), (90, 20, 7, 12)], []), ([(46, 50, 22, 30)], []), ([(50, 48, 16, 22)], []),
                          ([(52, 46, 9, 12)], []), _E]),
    # three identical slices: every candidate of slice 0 has a twin on slice 2 at the same distance from a click on slice 1
    "sym3": ((40, 48), [([(20, 24, 8, 10)], [])] * 3),
    # one small object on each of three slices: a click clears its slice
    "stop4": ((40, 48), [([(12, 14, 7, 7)], []), ([(20, 30, 7, 7)], []), ([(26, 18, 7, 7)], []), _E]),
    # two voxels: the erosion leaves nothing, the mean lies at .5 along z (floor 1, odd) and along x (floor 10, even)
    "tiny_a": ((40, 48), [_E, ([], [(10, 10, 10, 10)]), ([], [(10, 11, 10, 11)]), _E]),
    # ... at .5 along z (floor 0, even) and along x (floor 11, odd)
    "tiny_b": ((40, 48), [([], [(10, 11, 10, 11)]), ([], [(10, 12, 10, 12)]), _E, _E]),
    # four slices for a patch of six: the last two patch slices are padding
    "shallow4": ((40, 48), [_E, ([(20, 22, 12, 14)], []), ([(20, 22, 14, 16)], []), ([(22, 24, 9, 11)], [])]),
    "none4": ((40, 48), [_E] * 4),
    "all4": ((40, 48), [([], [(0, 0, 39, 47)])] * 4),
}

# rank_draw(2128, 5917): after the foreground click of draw 0 on patch slice 0 of "multi", candidate 2128 of the 5917 left
# lies on patch slice 2 within `step` of that click in the plane
FG_NEAR_DRAW = 1544649385
_FG = [0, LAST, 1 << 31, 12345]
_BG = [1 << 31, 0, LAST, 3 << 30]


def _rows(fg=_FG, bg=_BG, n_fg=4, n_bg=4):
    return [[n_fg, n_bg, strategy, 0] + list(fg) + list(bg) for strategy in (1, 3)]


# id, volume, centre (cz, cy, cx), patch depth D, crop (ch, cw), parameters, click_tab rows
RECORDS = [
    # the crop is clamped into the far (y, x) corner; foreground draw 1 lands within `step` of click 0 on another slice
    ("multi", "v100", (4, 90, 95), 6, (96, 100), REF_CLICKS, _rows(fg=[0, FG_NEAR_DRAW, LAST, 12345])),
    ("multi_small", "v100", (4, 90, 95), 6, (96, 100), SMALL_CLICKS, _rows()),
    ("sym", "sym3", (1, 20, 24), 3, (40, 48), REF_CLICKS, _rows()),
    ("stop", "stop4", (2, 20, 24), 4, (40, 48), REF_CLICKS, _rows()),
    ("tiny_a", "tiny_a", (2, 16, 20), 4, (32, 40), REF_CLICKS, _rows()),
    ("tiny_b", "tiny_b", (2, 16, 20), 4, (32, 40), REF_CLICKS, _rows()),
    ("shallow", "shallow4", (2, 20, 24), 6, (36, 44), REF_CLICKS, _rows()),
    ("none", "none4", (2, 16, 20), 4, (32, 40), REF_CLICKS, _rows()),
    ("all", "all4", (2, 20, 24), 4, (36, 44), REF_CLICKS, _rows()),
]
