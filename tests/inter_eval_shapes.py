"""Masks and toy predictors of the interactive-evaluation tests, built from a few integers (no generator): the fixture
generator (tests/golden/make_inter_eval_fixtures.py), the host tests and the GPU tests rebuild the same arrays from the specs
that tests/golden/ref_inter_eval.json records.

A mask spec is a list of [op, primitive, integers...]: op "+" sets, "-" clears, in order.  Primitives:
  ellipse cy cx ry rx     (y - cy)^2 rx^2 + (x - cx)^2 ry^2 <= ry^2 rx^2
  rect    y0 y1 x0 x1     rows y0 .. y1 - 1, columns x0 .. x1 - 1
  ring    cy cx ro ri     ri^2 < (y - cy)^2 + (x - cx)^2 <= ro^2"""
import numpy as np


def primitive(shape, name, *v):
    yy, xx = np.ogrid[:shape[0], :shape[1]]
    yy, xx = yy.astype(np.int64), xx.astype(np.int64)
    if name == "ellipse":
        cy, cx, ry, rx = v
        return (yy - cy) ** 2 * rx * rx + (xx - cx) ** 2 * ry * ry <= ry * ry * rx * rx
    if name == "rect":
        y0, y1, x0, x1 = v
        return (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
    if name == "ring":
        cy, cx, ro, ri = v
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        return (d2 <= ro * ro) & (d2 > ri * ri)
    raise ValueError(name)


def build(shape, spec):
    """uint8 {0, 1} mask [h, w] of a spec."""
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


def two_ellipses(shape):
    """The toy object: two overlapping ellipses scaled to the slice."""
    h, w = shape
    return [["+", "ellipse", (2 * h) // 5, (2 * w) // 5, h // 4, w // 5],
            ["+", "ellipse", (3 * h) // 5, (5 * w) // 8, h // 6, w // 4]]


def disc_prediction(shape, fg, bg, r_fg, r_bg):
    """The toy predictor: the union of discs of radius r_fg around the foreground clicks minus discs of radius r_bg around the
    background clicks."""
    spec = [["+", "ellipse", int(y), int(x), r_fg, r_fg] for y, x in fg] + [["-", "ellipse", int(y), int(x), r_bg, r_bg] for y, x in bg]
    return build(shape, spec)


def spiral(h, w):
    """A one-pixel-wide spiral with one-pixel gaps between its turns, walked inwards from the corner: a single 4-connected
    component whose union-find needs many rounds.  uint8 [h, w]."""
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


def resize_nearest(pred, src_hw):
    """The evaluator's nearest resize: pixel (y, x) of the [src_h, src_w] result reads pred[y * H // src_h, x * W // src_w]."""
    h, w = pred.shape
    ys = np.arange(src_hw[0], dtype=np.int64) * h // src_hw[0]
    xs = np.arange(src_hw[1], dtype=np.int64) * w // src_hw[1]
    return pred[ys][:, xs]
