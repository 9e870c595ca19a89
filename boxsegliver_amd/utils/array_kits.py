"""Array helpers the volume evaluator needs -- host-side mirror of the reference's utils/array_kits.py
(`get_largest_component` :357-384, `merge_labels`, `bbox_to_shape`)."""
import math

import numpy as np
from scipy import ndimage as ndi


def merge_labels(masks, merges):
    """utils/array_kits.py `merge_labels`: out = index (1-based) of the group of `merges` a label falls in; a group
    is an int, a list of ints, or -1 / [-1, ...] which collects "everything else" into 0."""
    out = np.zeros_like(masks, dtype=np.uint8)
    for i, group in enumerate(merges):
        if isinstance(group, (int, np.integer)):
            group = [int(group)]
        elif not isinstance(group, (list, tuple)):
            raise ValueError("Only integer or list is accepted, but got {}(type {}) in merges[{}]"
                             .format(group, type(group), i))
        for lab in group:
            out[masks == lab] = i
    return out


def get_largest_component(inputs, rank, connectivity=1):
    """Largest connected component (int8 0/1 array); a zero array stays zero (utils/array_kits.py:357-384).
    Ties resolve like np.argsort: the component with the larger label id."""
    struct = ndi.generate_binary_structure(rank, connectivity)
    res = np.asarray(inputs).astype(bool)
    if np.count_nonzero(res) == 0:
        return np.zeros_like(inputs, dtype=np.int8)
    labeled, _ = ndi.label(res, struct)
    areas = np.bincount(labeled.flat)[1:]
    order = np.argsort(areas)
    return merge_labels(labeled, [-1, int(order[-1]) + 1])


def match_components(res_sizes, ref_sizes, pairs, thresh):
    """The matching rule of utils/array_kits.py:920-984 on component tables: res_sizes [n_res] and ref_sizes [n_ref] the
    voxel counts of the result and reference objects (object id = index + 1), pairs rows (ref_id, res_id, overlap > 0), one
    per pair of objects that share voxels.  Returns {ref_id: [res_id, score]}.

    The score of a pair is 2 * overlap / (size_ref + size_res): the reference names it `iou` but computes medpy's Dice
    coefficient, and so does this.  Reference objects are walked in id order.  One whose candidates are a single result
    object is decided at once: matched if that object is still unused and scores >= thresh, else unmatched for good.  Those
    with several candidates wait; then, until none is left: the used result objects leave every waiting set, empty sets are
    dropped, the rest is stable-sorted by set size, and the first object tries its candidates in decreasing overlap (lowest
    result id on ties) until one scores >= thresh; it is dropped whether or not one did."""
    res_sizes, ref_sizes = np.asarray(res_sizes), np.asarray(ref_sizes)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]                    # by (ref_id, res_id)

    def score(ref_id, res_id, overlap):
        return 2.0 * overlap / float(int(ref_sizes[ref_id - 1]) + int(res_sizes[res_id - 1]))

    mapping, used, waiting = {}, set(), []
    starts = np.flatnonzero(np.r_[True, pairs[1:, 0] != pairs[:-1, 0]]) if len(pairs) else []
    for lo, hi in zip(starts, list(starts[1:]) + [len(pairs)]):
        ref_id = int(pairs[lo, 0])
        cands = {int(r): int(o) for _, r, o in pairs[lo:hi]}                 # ascending result id
        if len(cands) > 1:
            waiting.append((ref_id, cands))
            continue
        (res_id, overlap), = cands.items()
        if res_id not in used:
            s = score(ref_id, res_id, overlap)
            if s >= thresh:
                mapping[ref_id] = [res_id, s]
                used.add(res_id)
    while True:
        waiting = [(ref_id, {r: o for r, o in cands.items() if r not in used}) for ref_id, cands in waiting]
        waiting = sorted((w for w in waiting if w[1]), key=lambda w: len(w[1]))
        if not waiting:
            break
        ref_id, cands = waiting[0]
        for res_id in sorted(cands, key=lambda r: (-cands[r], r)):
            s = score(ref_id, res_id, cands[res_id])
            if s >= thresh:
                mapping[ref_id] = [res_id, s]
                used.add(res_id)
                break
        waiting = waiting[1:]
    return mapping


def distinct_binary_object_correspondences(result, reference, iou_thresh=0.5, connectivity=1):
    """utils/array_kits.py:883-984: label the objects of two binary volumes and match reference objects to result objects
    (match_components; `iou_thresh` is a threshold on the Dice coefficient of two objects, as in the reference).  Returns
    (labeled_res, labeled_ref, n_res, n_ref, mapping), mapping = {ref_id: [res_id, score]}.  Only connectivity 1 (faces)
    is built."""
    if connectivity != 1:
        raise ValueError("only connectivity 1 is supported, got {}".format(connectivity))
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    assert result.shape == reference.shape
    struct = ndi.generate_binary_structure(result.ndim, connectivity)
    labeled_res, n_res = ndi.label(result, struct)
    labeled_ref, n_ref = ndi.label(reference, struct)
    both = (labeled_res > 0) & (labeled_ref > 0)
    keys, overlaps = np.unique(labeled_ref[both].astype(np.int64) * (n_res + 1) + labeled_res[both], return_counts=True)
    pairs = np.stack([keys // (n_res + 1), keys % (n_res + 1), overlaps], axis=1)
    mapping = match_components(np.bincount(labeled_res.ravel(), minlength=n_res + 1)[1:],
                               np.bincount(labeled_ref.ravel(), minlength=n_ref + 1)[1:], pairs, iou_thresh)
    return labeled_res, labeled_ref, n_res, n_ref, mapping


def bbox_to_shape(bbox):
    """(x1, y1, z1, x2, y2, z2) inclusive -> (d, h, w)  (utils/array_kits.py `bbox_to_shape`)."""
    ndim = len(bbox) // 2
    return tuple(int(bbox[i + ndim]) - int(bbox[i]) + 1 for i in range(ndim))[::-1]


def bbox_to_slices(bbox):
    """(x1, y1, [z1,] x2, y2[, z2]) inclusive -> index slices in array order ([z,] y, x) (utils/array_kits.py:177-195)."""
    if len(bbox) % 2 != 0:
        raise ValueError("`bbox` should have even number of elements, got {}".format(len(bbox)))
    ndim = len(bbox) // 2
    return tuple(slice(int(bbox[i]), int(bbox[i + ndim]) + 1) for i in reversed(range(ndim)))


def bbox_from_mask(mask, mask_values=1):
    """utils/array_kits.py:85-151 (without min_shape / padding): tight box of the voxels whose value is in mask_values,
    (x1, y1, x2, y2) or (x1, y1, z1, x2, y2, z2), both corners INSIDE the object; zeros for an empty mask."""
    mask = np.asarray(mask)
    values = np.atleast_1d(mask_values)
    sel = np.isin(mask, values)
    if not sel.any():
        return np.zeros(shape=(mask.ndim * 2,))
    lo, hi = [], []
    for ax in range(mask.ndim):
        proj = np.where(sel.any(axis=tuple(a for a in range(mask.ndim) if a != ax)))[0]
        lo.append(int(proj[0]))
        hi.append(int(proj[-1]))
    return np.array(lo[::-1] + hi[::-1])


def extract_region(mask):
    """utils/array_kits.py:263-340 with the defaults the exporter uses (align 1, padding 0): box of the non-zero voxels,
    (x1, y1, [z1,] x2, y2[, z2]) inclusive."""
    return bbox_from_mask(np.asarray(mask) != 0, 1)


def compute_robust_moments(binary_image, isotropic=False, indexing="ij", min_std=0.):
    """utils/array_kits.py:387-440: median of the foreground coordinates and 1.4826 x median absolute deviation per
    axis (or of the radial distance when isotropic); (-1, ...) for an empty image."""
    binary_image = np.asarray(binary_image)
    ndim = binary_image.ndim
    points = np.asarray(np.nonzero(binary_image)).astype(np.float32)
    if points.shape[1] == 0:
        return np.array([-1.0] * ndim, dtype=np.float32), np.array([-1.0] * ndim, dtype=np.float32)
    points = np.transpose(points)
    center = np.median(points, axis=0)
    if isotropic:
        mad = np.array([np.median(np.linalg.norm(points - center, axis=1))] * ndim)
    else:
        mad = np.median(np.absolute(points - center), axis=0)
    std_dev = np.maximum(1.4826 * mad, [min_std] * ndim)
    if not indexing or indexing == "xy":
        return center[::-1], std_dev[::-1]
    if indexing == "ij":
        return center, std_dev
    raise ValueError("Valid values for `indexing` are 'xy' and 'ij'.")


def xiaolinwu_line(x0, y0, x1, y1):
    """utils/array_kits.py `xiaolinwu_line`: the pixels (xs, ys) of Xiaolin Wu's line from (x0, y0) to (x1, y1), one per step
    along the major axis (the first pixel of each anti-aliased pair), ordered from the end with the smaller major
    coordinate; `forward` is False when that end is (x1, y1).  The same float64 arithmetic as the reference, so the
    floors fall on the same pixels."""
    if x0 == x1 and y0 == y1:
        raise ValueError("Must be different points, but the same ({}) vs ({})".format(x0, y0))
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:                                   # walk along y: swap the roles of the axes
        x0, y0, x1, y1 = y0, x0, y1, x1
    forward = not x0 > x1
    if not forward:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    gradient = 1. if dx == 0 else 1. * dy / dx
    a_major = round(x0)
    intery = y0 + gradient * (a_major - x0)
    majors, minors = [a_major], [math.floor(intery)]
    intery += gradient
    b_major = round(x1)
    b_minor = math.floor(y1 + gradient * (b_major - x1))
    for m in range(a_major + 1, b_major):
        majors.append(m)
        minors.append(math.floor(intery))
        intery += gradient
    majors.append(b_major)
    minors.append(b_minor)
    return (minors, majors, forward) if steep else (majors, minors, forward)
