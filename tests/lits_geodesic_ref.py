"""Restatement of the geodesic click guide (`--geodesic_guide`; include/unetk.h "geodesic click guides").

The reference calls GeodisTK on the host (DataLoader/NF/input_pipeline_g_simply.py:471-496, entry/main_eval.py:205-220); this
project DEFINES the distance instead: the float32 shortest path on the 8-connected grid under the step cost
sqrt(s2 + (I[p] - I[q])^2), s2 = 1 axial / 2 diagonal, a path's length being the left-to-right float32 sum of its costs.
Two solvers state it independently -- a heap Dijkstra and a Jacobi relaxation, every operation a numpy float32 one -- and the
host test shows they agree bit for bit, which is the claim that the fixed point does not depend on the order."""
import heapq

import numpy as np

import lits3d_ref

F = np.float32
NEIGHBOURS = ((-1, -1, 2.0), (-1, 0, 1.0), (-1, 1, 2.0), (0, -1, 1.0), (0, 1, 1.0), (1, -1, 2.0), (1, 0, 1.0), (1, 1, 2.0))


# ------------------------------------------------------------------------------------------------- seeds
def seed_index(y, ch, h, extent):
    """:483 `int(y / ch * H / 2)` in float32 -- each operation rounded, truncated toward zero -- clamped into the grid."""
    g = F(F(F(y) / F(ch)) * F(h)) / F(2.0)
    return int(min(max(int(g), 0), extent - 1))


def seeds_of(pts, cnt, crop_hw, out_hw):
    """The grid seeds [(gy, gx)] of one kind's click list (pts [K, 2] relative to the crop box, the first `cnt` valid)."""
    hh, hw = (out_hw[0] + 1) // 2, (out_hw[1] + 1) // 2
    k = min(max(int(cnt), 0), len(pts))
    return [(seed_index(int(p[0]), crop_hw[0], out_hw[0], hh), seed_index(int(p[1]), crop_hw[1], out_hw[1], hw)) for p in pts[:k]]


# ------------------------------------------------------------------------------------------------- step costs
def step_costs(field):
    """cost[k][y, x] = c((y, x), (y + dy_k, x + dx_k)) in float32 (+inf where the neighbour leaves the grid)."""
    field = np.asarray(field, F)
    h, w = field.shape
    pad = np.full((h + 2, w + 2), np.nan, F)
    pad[1:-1, 1:-1] = field
    out = []
    for dy, dx, s2 in NEIGHBOURS:
        nb = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        with np.errstate(invalid="ignore"):
            di = (nb - field).astype(F)
            c = np.sqrt((F(s2) + (di * di).astype(F)).astype(F)).astype(F)
        out.append(np.where(np.isnan(nb), F(np.inf), c).astype(F))
    return out


# ------------------------------------------------------------------------------------------------- the two solvers
def dijkstra(field, seeds):
    """Heap Dijkstra in strict float32: D[q] = fl(D[p] + c(p, q)) along the tree.  No seed: zeros (false_fn)."""
    field = np.asarray(field, F)
    h, w = field.shape
    if not seeds:
        return np.zeros((h, w), F)
    cost = step_costs(field)
    dist = np.full((h, w), np.inf, F)
    heap = []
    for y, x in seeds:
        dist[y, x] = F(0)
        heap.append((0.0, y, x))
    heapq.heapify(heap)
    done = np.zeros((h, w), bool)
    while heap:
        d, y, x = heapq.heappop(heap)
        if done[y, x]:
            continue
        done[y, x] = True
        dp = dist[y, x]
        for k, (dy, dx, _) in enumerate(NEIGHBOURS):
            qy, qx = y + dy, x + dx
            if 0 <= qy < h and 0 <= qx < w and not done[qy, qx]:
                cand = F(dp + cost[k][y, x])
                if cand < dist[qy, qx]:
                    dist[qy, qx] = cand
                    heapq.heappush(heap, (float(cand), qy, qx))
    return dist


def jacobi(field, seeds, max_sweeps=None):
    """Jacobi relaxation from +inf in strict float32 -> (D, sweeps that lowered something).  Every sweep reads the previous
    sweep's D only."""
    field = np.asarray(field, F)
    h, w = field.shape
    if not seeds:
        return np.zeros((h, w), F), 0
    cost = step_costs(field)
    dist = np.full((h, w), np.inf, F)
    for y, x in seeds:
        dist[y, x] = F(0)
    sweeps = 0
    limit = h * w if max_sweeps is None else max_sweeps
    while sweeps < limit:
        pad = np.full((h + 2, w + 2), np.inf, F)
        pad[1:-1, 1:-1] = dist
        new = dist
        for k, (dy, dx, _) in enumerate(NEIGHBOURS):
            nb = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            new = np.minimum(new, (nb + cost[k]).astype(F))              # c(q, p) = c(p, q): the square is symmetric
        if np.array_equal(new, dist):
            break
        dist = new
        sweeps += 1
    return dist, sweeps


# ------------------------------------------------------------------------------------------------- the guide
def resize(dist, out_hw):
    """lits3d_ref.resize_bilinear (align_corners, float32 coordinates, float64 lerps) of one field."""
    return lits3d_ref.resize_bilinear(np.asarray(dist, np.float64)[None], out_hw)[0]


def guide(base, pts, cnt, crop_hw, out_hw, flips=(0, 0), channels=2):
    """(guide float64 [H, W, channels], dist float32 [2, hh, hw]) of one sample; flips = (left/right, up/down)."""
    dist = np.stack([dijkstra(base, seeds_of(pts[kind], cnt[kind], crop_hw, out_hw)) for kind in range(2)])
    g = np.stack([resize(dist[kind], out_hw) for kind in range(2)], axis=-1)
    if flips[0]:
        g = g[:, ::-1]
    if flips[1]:
        g = g[::-1]
    if channels == 1:
        g = g[..., :1] - g[..., 1:]
    return np.ascontiguousarray(g), dist


# ------------------------------------------------------------------------------------------------- synthetic fields
def field_normal(h, w, seed=0):
    return np.random.default_rng(seed).standard_normal((h, w)).astype(F)


def field_constant(h, w, value=0.75):
    return np.full((h, w), value, F)


def field_step(h, w, height=3.0):
    """A vertical step edge in the middle."""
    f = np.zeros((h, w), F)
    f[:, w // 2:] = height
    return f


def field_maze(n=33, height=1000.0):
    """A square spiral corridor of width 1 between walls of `height`: from the corner (0, 0) the cheap way to the centre
    winds through ~n^2 / 2 pixels, so a relaxation needs far more than n sweeps."""
    f = np.full((n, n), height, F)
    y, x, dy, dx = 0, 0, 0, 1
    f[0, 0] = 0
    while True:
        moved = False
        for _ in range(4):
            ny, nx = y + dy, x + dx
            ahead_y, ahead_x = ny + dy, nx + dx
            free = 0 <= ny < n and 0 <= nx < n and f[ny, nx] != 0
            # stop one short of a corridor already cut: the wall between two turns stays
            if free and not (0 <= ahead_y < n and 0 <= ahead_x < n and f[ahead_y, ahead_x] == 0):
                y, x = ny, nx
                f[y, x] = 0
                moved = True
                break
            dy, dx = dx, -dy                                             # turn right
        if not moved:
            return f
