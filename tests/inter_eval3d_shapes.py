"""Volumes and toy predictors of the 3-D interactive-evaluation tests, built from a few integers (no generator): the
fixture generator (tests/golden/make_inter_eval3d_fixtures.py), the host tests and the GPU tests rebuild the same arrays from
the specs that tests/golden/ref_inter_eval3d.json records.

A mask spec is a list of [op, primitive, integers...]: op "+" sets, "-" clears, in order.  Primitives:
  ellipsoid cz cy cx rz ry rx        (z - cz)^2 ry^2 rx^2 + (y - cy)^2 rz^2 rx^2 + (x - cx)^2 rz^2 ry^2 <= rz^2 ry^2 rx^2
  box       z0 z1 y0 y1 x0 x1        slices z0 .. z1 - 1, rows y0 .. y1 - 1, columns x0 .. x1 - 1
  shell     cz cy cx rz ry rx tz t   the ellipsoid (rz, ry, rx) without the ellipsoid (rz - tz, ry - t, rx - t); an inner
                                     ellipsoid with a radius < 1 is empty"""
import numpy as np


def primitive(shape, name, *v):
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    zz, yy, xx = zz.astype(np.int64), yy.astype(np.int64), xx.astype(np.int64)
    if name == "ellipsoid":
        cz, cy, cx, rz, ry, rx = v
        return ((zz - cz) ** 2 * ry * ry * rx * rx + (yy - cy) ** 2 * rz * rz * rx * rx + (xx - cx) ** 2 * rz * rz * ry * ry
                <= rz * rz * ry * ry * rx * rx)
    if name == "box":
        z0, z1, y0, y1, x0, x1 = v
        return (zz >= z0) & (zz < z1) & (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
    if name == "shell":
        cz, cy, cx, rz, ry, rx, tz, t = v
        outer = primitive(shape, "ellipsoid", cz, cy, cx, rz, ry, rx)
        if min(rz - tz, ry - t, rx - t) < 1:
            return outer
        return outer & ~primitive(shape, "ellipsoid", cz, cy, cx, rz - tz, ry - t, rx - t)
    raise ValueError(name)


def build(shape, spec):
    """uint8 {0, 1} mask [d, h, w] of a spec."""
    m = np.zeros(tuple(shape), dtype=bool)
    for item in spec:
        p = primitive(shape, item[1], *item[2:])
        if item[0] == "+":
            m |= p
        elif item[0] == "-":
            m &= ~p
        else:
            raise ValueError(item[0])
    return m.astype(np.uint8)


def two_ellipsoids(shape):
    """The toy object: two overlapping ellipsoids scaled to the case."""
    d, h, w = shape
    return [["+", "ellipsoid", (2 * d) // 5, (2 * h) // 5, (2 * w) // 5, max(d // 3, 1), h // 4, w // 5],
            ["+", "ellipsoid", (3 * d) // 5, (3 * h) // 5, (5 * w) // 8, max(d // 4, 1), h // 6, w // 4]]


def ball_prediction(shape, fg, bg, r_fg, r_bg):
    """The toy predictor: the union of ellipsoids of radii r_fg = (rz, r, r) around the foreground clicks minus ellipsoids of
    radii r_bg around the background clicks."""
    spec = [["+", "ellipsoid", int(z), int(y), int(x), r_fg[0], r_fg[1], r_fg[1]] for z, y, x in fg]
    spec += [["-", "ellipsoid", int(z), int(y), int(x), r_bg[0], r_bg[1], r_bg[1]] for z, y, x in bg]
    return build(shape, spec)


def spiral2d(h, w):
    """A one-pixel-wide spiral with one-pixel gaps between its turns, walked inwards from the corner.  uint8 [h, w]."""
    m = np.zeros((h, w), dtype=np.uint8)

    def free(y, x):
        return not (0 <= y < h and 0 <= x < w) or not m[y, x]

    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and free(ny + dy, nx + dx):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return m


def spiral(d, h, w):
    """A one-voxel-wide 3-D spiral: the 2-D spiral on every even slice, neighbouring spirals joined by the single voxel (0, 0)
    of the odd slice between them -- ONE 6-connected component whose union-find needs many rounds.  uint8 [d, h, w]."""
    m = np.zeros((d, h, w), dtype=np.uint8)
    m[0::2] = spiral2d(h, w)
    m[1::2, 0, 0] = 1
    return m
