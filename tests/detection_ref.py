"""Per-lesion detection restated for the tests (no GPU): labelling, pair counting and the matching rule of the reference's
utils/array_kits.distinct_binary_object_correspondences / loss_metrics.tumor_detection_metrics, written from their
description and kept apart from boxsegliver_amd.utils.array_kits.

The reference function does run in the build container with two shims -- `np.bool` aliased to bool and a stand-in for
`medpy.metric.dc`, dc(a, b) = 2 |a & b| / (|a| + |b|) -- and tests/golden/make_detection_fixtures.py records what it gives
in tests/golden/ref_detection.npz (`reference_records` reads it).  test_ref_detection_host.py holds this restatement and
array_kits to those records, test_gpu_detection.py the device tables.  That pins the matching rule (the labelling, which
reference object gets which result object, in which order); it does not pin medpy's Dice, which is the stand-in's.

The reference keeps the candidates of a reference object that overlaps several result objects in a container of its own.
WaitingSet is that container, with its quirks:
  * a dict from result id to overlap count, filled in ascending result id (the order np.unique returns them);
  * subtraction removes ids and keeps the insertion order of the rest;
  * pop returns the FIRST key that holds the maximum count (so the lowest result id on ties) and raises KeyError when
    nothing is left;
  * popping does not shrink the length the size sort and the emptiness test see: that length is fixed when the set is built.
"""
import json
import os

import numpy as np
import scipy.ndimage as ndi


class WaitingSet(object):
    def __init__(self, ids=(), counts=()):
        assert len(ids) == len(counts)
        self.counts = {}
        for k, v in zip(ids, counts):
            self.counts[int(k)] = int(v)
        self.length = len(self.counts)           # what len() and truth see, pops or not

    def __len__(self):
        return self.length

    def __sub__(self, used):
        rest = dict(self.counts)
        for k in used:
            rest.pop(k, None)
        return WaitingSet(list(rest.keys()), list(rest.values()))

    def pop(self):
        if not self.counts:
            raise KeyError
        best = None
        for k, v in self.counts.items():         # first key with the maximum
            if best is None or v > self.counts[best]:
                best = k
        del self.counts[best]
        return best


def label_tables(result, reference):
    """(labeled_res, labeled_ref, res_sizes, ref_sizes, pairs): scipy's 6-connected labels, object sizes by np.bincount and
    the rows (ref_id, res_id, overlap) of every pair of objects sharing a voxel by np.unique, sorted by (ref_id, res_id)."""
    struct = ndi.generate_binary_structure(3, 1)
    lres, n_res = ndi.label(np.asarray(result) != 0, struct)
    lref, n_ref = ndi.label(np.asarray(reference) != 0, struct)
    res_sizes = np.bincount(lres.ravel(), minlength=n_res + 1)[1:].astype(np.int64)
    ref_sizes = np.bincount(lref.ravel(), minlength=n_ref + 1)[1:].astype(np.int64)
    both = (lres > 0) & (lref > 0)
    rows = np.stack([lref[both], lres[both]], axis=1).astype(np.int64).reshape(-1, 2)
    if len(rows):
        uniq, counts = np.unique(rows, axis=0, return_counts=True)
        pairs = np.concatenate([uniq, counts[:, None]], axis=1).astype(np.int64)
    else:
        pairs = np.zeros((0, 3), np.int64)
    return lres, lref, res_sizes, ref_sizes, pairs


def correspondences(result, reference, thresh=0.5, stats=None):
    """(n_res, n_ref, mapping {ref_id: [res_id, score]}) of two binary volumes.  stats, a dict, receives "waiting": how many
    reference objects reached the several-candidates loop."""
    lres, lref, res_sizes, ref_sizes, _ = label_tables(result, reference)
    n_res, n_ref = len(res_sizes), len(ref_sizes)

    def dice(ref_id, res_id):
        a, b = lref == ref_id, lres == res_id
        return 2.0 * np.count_nonzero(a & b) / float(np.count_nonzero(a) + np.count_nonzero(b))

    mapping, used, waiting = {}, set(), []
    for ref_id in range(1, n_ref + 1):
        ids, counts = np.unique(lres[lref == ref_id], return_counts=True)
        keep = ids != 0
        ids, counts = ids[keep], counts[keep]
        if len(ids) == 1:
            res_id = int(ids[0])
            if res_id not in used:
                s = dice(ref_id, res_id)
                if s >= thresh:
                    mapping[ref_id] = [res_id, s]
                    used.add(res_id)
        elif len(ids) > 1:
            waiting.append((ref_id, WaitingSet(ids, counts)))
    if stats is not None:
        stats["waiting"] = len(waiting)
    while True:
        waiting = [(ref_id, cands - used) for ref_id, cands in waiting]
        waiting = [w for w in waiting if w[1]]
        waiting = sorted(waiting, key=lambda w: len(w[1]))
        if len(waiting) == 0:
            break
        ref_id, cands = waiting[0]
        while True:
            try:
                res_id = cands.pop()
            except KeyError:
                break
            s = dice(ref_id, res_id)
            if s >= thresh:
                mapping[ref_id] = [res_id, s]
                used.add(res_id)
                break
        waiting = waiting[1:]
    return n_res, n_ref, mapping


def detection_metrics(result, reference, thresh=0.5):
    n_res, n_ref, mapping = correspondences(result, reference, thresh)
    tp = len(mapping)
    return {"tp": tp, "fp": n_res - tp, "pos": n_ref,
            "precision": tp / n_res if n_res != 0 else np.inf,
            "recall": tp / n_ref if n_ref != 0 else np.inf}


def blob(rng, shape, density, sigma=1.0):
    """Thresholded smoothed noise with the given fraction of object voxels."""
    x = ndi.gaussian_filter(rng.random(shape), sigma)
    return x > np.quantile(x, 1.0 - density)


def reference_records():
    """tests/golden/ref_detection.npz as [(name, result bool [D, H, W], reference bool [D, H, W], n_res, n_ref, {thresh: rows})],
    rows int64 [m, 5] = (reference object's first voxel, result object's first voxel, intersection, reference size, result
    size) of the matched pairs in the order the reference decided them; first voxels are row-major flat indices."""
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_detection.npz"))
    names, off, moff = json.loads(str(f["names"])), f["bit_offsets"], f["match_offsets"]
    out = []
    for c, name in enumerate(names):
        shape = tuple(int(v) for v in f["shapes"][c])
        n = int(np.prod(shape))
        vols = [np.unpackbits(f["bits"][off[2 * c + k]:off[2 * c + k + 1]])[:n].reshape(shape).astype(bool) for k in range(2)]
        rows = {float(t): f["matches"][moff[3 * c + k]:moff[3 * c + k + 1]] for k, t in enumerate(f["thresholds"])}
        out.append((name, vols[0], vols[1], int(f["counts"][c, 0]), int(f["counts"][c, 1]), rows))
    return out


def first_voxels(labeled, n):
    """Row-major flat index of the first voxel of objects 1 .. n of a labelled volume."""
    ids, first = np.unique(labeled.ravel(), return_index=True)
    assert ids[ids > 0].tolist() == list(range(1, n + 1))
    return first[ids > 0].astype(np.int64)
