"""The restatement of `unetk_boundary_weights3d` (include/unetk.h) in numpy and scipy, and the seeded label
volumes of its tests.

  ring    27 shifted comparisons on an edge-padded array: a voxel whose 3x3x3 neighbourhood, clipped to the volume, holds another label
  d2      scipy.ndimage.distance_transform_edt(~ring, sampling=(K, 1, 1)), squared and rounded: the float64 root of an integer below
          2^31 squares back to it to well under 1/2
  map     float64: exp(-float32(d) / 25) + 1, scaled to mean 1 per sample
A volume without a ring voxel has d2 = -1 and weights 1 (the project's rule; scipy's answer for an input without zeros is not used)."""
import itertools

import numpy as np


def ring(lab):
    """lab [D, H, W] -> bool [D, H, W]."""
    lab = np.asarray(lab)
    d, h, w = lab.shape
    p = np.pad(lab, 1, mode="edge")                   # an edge-padded neighbour repeats a label of the neighbourhood: adds nothing
    out = np.zeros(lab.shape, bool)
    for dz, dy, dx in itertools.product(range(3), repeat=3):
        out |= p[dz:dz + d, dy:dy + h, dx:dx + w] != lab
    return out


def edt(r, k):
    """float64 distances to the nearest voxel of r [D, H, W] (which holds one), z counted k-fold."""
    from scipy.ndimage import distance_transform_edt
    return distance_transform_edt(~r, sampling=(k, 1, 1))


def d2_one(lab, k=1):
    """int64 [D, H, W]: the exact squared distances of one sample, -1 everywhere without a ring voxel."""
    r = ring(lab)
    if not r.any():
        return np.full(r.shape, -1, np.int64)
    d = edt(r, k)
    return np.rint(d * d).astype(np.int64)


def d2(labels, k=1):
    return np.stack([d2_one(lab, k) for lab in labels])


def weights(labels, k=1):
    """float64 [N, D, H, W]: the normalised map of a batch."""
    out = []
    for lab in labels:
        q = d2_one(lab, k)
        if q[0, 0, 0] < 0:
            out.append(np.ones(q.shape))
            continue
        dist = np.sqrt(q.astype(np.float64)).astype(np.float32).astype(np.float64)
        w = np.exp(-dist / 25.0) + 1.0
        out.append(w * (w.size / w.sum()))
    return np.stack(out)


def d2_brute(lab, k=1):
    """Voxel by voxel over every ring voxel; tiny volumes only."""
    lab = np.asarray(lab)
    d, h, w = lab.shape
    r = np.zeros(lab.shape, bool)
    for z, y, x in np.ndindex(*lab.shape):
        nb = lab[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
        r[z, y, x] = (nb != lab[z, y, x]).any()
    pts = np.argwhere(r).astype(np.int64)
    out = np.full(lab.shape, -1, np.int64)
    if len(pts) == 0:
        return r, out
    for z, y, x in np.ndindex(*lab.shape):
        out[z, y, x] = ((k * (pts[:, 0] - z)) ** 2 + (pts[:, 1] - y) ** 2 + (pts[:, 2] - x) ** 2).min()
    return r, out


def other_slice(lab):
    """bool [D, H, W]: voxels whose nearest ring voxel (K = 1) lies in another slice -- strictly nearer than every ring voxel of
    the voxel's own slice."""
    r = ring(lab)
    full = d2_one(lab, 1)
    own = np.full(full.shape, np.iinfo(np.int64).max, np.int64)
    for z in range(lab.shape[0]):
        if r[z].any():                                # a slice without one: every ring voxel lies in another slice
            dz = edt(r[z:z + 1], 1)[0]
            own[z] = np.rint(dz * dz).astype(np.int64)
    return full < own


def labels(shape, seed, n=1):
    """int32 [n, D, H, W] in {0, 1, 2}: two nested ellipsoids (class 1 around class 2) about a centre jittered in the plane,
    squeezed x2 along z and sitting on the first slice (odd samples: on the last), so that they close within the volume and
    the slices beyond find their nearest ring voxel in another slice; plus 0.2 % speckle of class 1."""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((n, d, h, w), np.int32)
    for i in range(n):
        cy, cx = ((s - 1) / 2.0 + rng.uniform(-0.1, 0.1) * s for s in (h, w))
        cz = 0.0 if i % 2 == 0 else d - 1.0
        rz, ry, rx = max(0.22 * d, 0.6), max(0.44 * h, 0.6), max(0.44 * w, 0.6)
        q = ((zz - cz) / rz) ** 2 + ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        out[i][q <= 1.0] = 1
        out[i][q <= 0.25] = 2
        out[i][rng.random(shape) < 0.002] = 1
    return out
