"""CPU: the stepped staging addresses of conv3x3_wgrad_kernel's plain tiles (csrc/conv_wgrad.hip, `issue_plain`) against the
per-tile form (`issue_general`), emulated on the host.  The kernel uses the stepped form for its 64 x 64 fp32 panel of plain 8 x 16
tiles; the arithmetic is the same for every plain geometry, so the narrower panels, the atrous and the stride-2 tiles are walked
too.

The kernel carries the next tile's (image, tile row, tile column) along and steps it, and adds a per-block piece offset to a
wave-uniform tile origin; the form it replaced derived everything from the tile index.  Both must name the same element for every
in-image piece and agree on which pieces read the zero page -- for splits that start in the middle of an image, cross image
boundaries, and end short.  This pins the arithmetic; the kernel itself is compared bit for bit on the device
(tests/test_gpu_conv_paths.py)."""
import pytest

M32 = 0xFFFFFFFF


def _geom(cit, cot, th, tw, s, dil):
    hwd = (tw - 1) * s + 2 * dil + 1
    halo = ((th - 1) * s + 2 * dil + 1) * hwd
    ppx, ppy = 256 // cit, 256 // cot
    return hwd, halo, ppx, ppy, (halo + ppx - 1) // ppx, th * tw // ppy


def _walk(cit, cot, th, tw, s, dil, n_img, h, w, hin, win, pb, xs, ys, ci0, co0, tps):
    hwd, halo, ppx, ppy, ni_x, ni_y = _geom(cit, cot, th, tw, s, dil)
    tiles_h, tiles_w = (h + th - 1) // th, (w + tw - 1) // tw
    total = n_img * tiles_h * tiles_w
    ximg_stride, yimg_stride = hin * win * xs, h * w * ys
    checked = 0
    for split in range((total + tps - 1) // tps):
        t_begin, t_end = split * tps, min(split * tps + tps, total)
        nx_tw, nx_th, nx_n = t_begin % tiles_w, (t_begin // tiles_w) % tiles_h, t_begin // (tiles_w * tiles_h)
        for tile in range(t_begin, t_end):
            tw_i, th_i, n = tile % tiles_w, (tile // tiles_w) % tiles_h, tile // (tiles_w * tiles_h)
            assert (tw_i, th_i, n) == (nx_tw, nx_th, nx_n), (split, tile)
            h0, w0 = th_i * th, tw_i * tw
            for j in range(ni_x + ni_y):
                for lane in (0, 1, 17, 31, 40, 63):
                    is_x = j < ni_x
                    if is_x:
                        lp, q = lane // (cit // 4), lane % (cit // 4)
                        pix = ppx * j + lp
                        rel_h, rel_w = (pix // hwd if pix < halo else 1 << 20), pix % hwd
                    else:
                        lp, q = lane // (cot // 4), lane % (cot // 4)
                        pix = ppy * (j - ni_x) + lp
                        rel_h, rel_w = pix // tw, pix % tw
                    # the per-tile form
                    gh = s * h0 - pb + rel_h if is_x else h0 + rel_h
                    gw = s * w0 - pb + rel_w if is_x else w0 + rel_w
                    ph, pw = (hin, win) if is_x else (h, w)
                    ok_old = 0 <= gh < ph and 0 <= gw < pw
                    a_old = (n * ximg_stride + (gh * pw + gw) * xs + ci0 + q * 4) if is_x else \
                        (n * yimg_stride + (gh * pw + gw) * ys + co0 + q * 4)
                    # the stepped form
                    hx, wx = s * h0 - pb, s * w0 - pb
                    xb = n * ximg_stride + (hx * win + wx) * xs
                    yb = n * yimg_stride + (h0 * w + w0) * ys
                    if is_x:
                        roff = 0 if rel_h >= 1 << 20 else (rel_h * win + rel_w) * xs + ci0 + q * 4
                    else:
                        roff = (rel_h * w + rel_w) * ys + co0 + q * 4
                    uh, uw = ((hx if is_x else h0) + rel_h) & M32, ((wx if is_x else w0) + rel_w) & M32   # unsigned compares
                    ok_new = uh < (hin if is_x else h) and uw < (win if is_x else w)
                    assert ok_old == ok_new, (tile, j, lane)
                    if ok_old:
                        assert a_old == (xb if is_x else yb) + roff, (tile, j, lane)
                    checked += 1
            nx_tw += 1
            if nx_tw == tiles_w:
                nx_tw, nx_th = 0, nx_th + 1
                if nx_th == tiles_h:
                    nx_th, nx_n = 0, nx_n + 1
    return checked


PLANES = [(2, 22, 40), (3, 8, 15), (1, 5, 7), (2, 16, 32), (1, 200, 1), (4, 9, 31)]


@pytest.mark.parametrize("cit,cot", [(64, 64), (64, 32), (32, 64), (32, 32)])
@pytest.mark.parametrize("tps", [1, 3, 7, 100])      # tiles per split: splits start mid-row, mid-image, cross images, end short
def test_plain_tiles(cit, cot, tps):
    for n, h, w in PLANES:     # x and dy are channel slices of wider buffers, the panel is not the first
        assert _walk(cit, cot, 8, 16, 1, 1, n, h, w, h, w, 1, 2 * cit + 8, cot + 4, cit, 0, tps) > 0


@pytest.mark.parametrize("plane", [(2, 20, 24), (3, 1, 1), (3, 2, 3)])
def test_atrous_tiles(plane):
    n, h, w = plane
    assert _walk(64, 64, 6, 16, 1, 2, n, h, w, h, w, 2, 64, 64, 0, 64, 5) > 0


@pytest.mark.parametrize("tw", [16, 12, 6])
def test_stride2_tiles(tw):
    # (N, Ho, Wo, Hin, Win, pad-before): even input extents pad 0, odd ones 1
    for n, ho, wo, hin, win, pb in [(2, 6, tw, 12, 2 * tw, 0), (2, 6, tw, 11, 2 * tw - 1, 1), (3, 5, tw + 3, 10, 2 * tw + 6, 0)]:
        assert _walk(32, 64, 4, tw, 2, 1, n, ho, wo, hin, win, pb, 32, 64, 0, 0, 4) > 0
