"""Lesion-matching fixtures pinned on the REFERENCE ITSELF (build container only): utils/array_kits.py
`distinct_binary_object_correspondences` run on small binary volume pairs at the thresholds 0.5, 0.3 and 0.1, written to
tests/golden/ref_detection.npz.

    python tests/golden/make_detection_fixtures.py     # needs the reference checkout; rewrites ref_detection.npz

WHAT IS PINNED is the matching rule: which reference object gets which result object, in which order, with the reference's
own labelling (scipy.ndimage.label), its candidate container and its loops.  WHAT IS NOT PINNED is medpy's Dice coefficient:
medpy is not installed, so `medpy.metric.dc` is the stand-in dc(a, b) = 2 |a & b| / (|a| + |b|) written below (0 for two
empty masks), which is what medpy documents.  The module also imports skimage (a stand-in from
make_propagation_fixtures.py; unused by the function) and says `np.bool`, which numpy 1.24 removed: it is aliased to bool.

Inputs: 24 seeded pairs of thresholded smoothed noise, at most 8 x 24 x 24, two thirds of them correlated (a shifted copy
cut and joined by other blobs), and hand-built layouts that put the one-to-many loop into each situation
tests/test_detection_host.py describes: a contested result object decided by set size, a set shrunk by a used candidate,
equal overlaps, equal set sizes, a largest overlap that fails the threshold, a used single candidate, and a set emptied by
earlier matches.  A layout is built from its pair table: plane 1 holds one strip of `overlap` voxels per pair, set in both
volumes; result objects are joined in plane 0 and padded there, reference objects in plane 2, so no other voxel is shared.

Recorded, free of label numbering: n_res and n_ref per pair of volumes, and per threshold the matched pairs in the order
the reference decided them, each as (first voxel of the reference object, first voxel of the result object -- row-major
flat indices --, intersection, reference size, result size).  The Dice score is the quotient of these integers."""
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_propagation_fixtures as mpf  # noqa: E402

THRESHOLDS = (0.5, 0.3, 0.1)
N_RANDOM, SEED = 24, 17


def _import_reference():
    mpf.STUBBED = ("skimage", "medpy")
    sys.meta_path.insert(0, mpf._StubFinder())
    if not hasattr(np, "bool"):
        np.bool = bool
    sys.path.insert(0, os.path.join(mpf.REF, "utils"))
    import array_kits

    def dc(a, b):
        a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
        total = np.count_nonzero(a) + np.count_nonzero(b)
        return 2.0 * np.count_nonzero(a & b) / float(total) if total else 0.0
    array_kits.mtr.dc = dc
    return array_kits


# ------------------------------------------------------------------------------------------------- inputs
def _blob(rng, shape, density, sigma):
    x = ndi.gaussian_filter(rng.random(shape), sigma)
    return x > np.quantile(x, 1.0 - density)


def random_pairs():
    rng = np.random.default_rng(SEED)
    for t in range(N_RANDOM):
        shape = (int(rng.integers(3, 9)), int(rng.integers(12, 25)), int(rng.integers(12, 25)))
        a = _blob(rng, shape, rng.uniform(0.04, 0.12), rng.uniform(1.0, 1.8))
        b = _blob(rng, shape, rng.uniform(0.04, 0.12), rng.uniform(1.0, 1.8))
        if t % 3 != 2:
            b = np.roll(a, tuple(int(s) for s in rng.integers(-1, 2, 3)), (0, 1, 2)) ^ b
        yield "random{:02d}".format(t), a, b


def layout(pairs, res_pad, ref_pad):
    """(result, reference) bool [3, 2 n_ref, n_res * bx] from rows (ref_id, res_id, overlap) and the voxels added to every
    object beyond its strips and joints.  Objects come out numbered as given: result objects by their column, reference objects
    by their row."""
    n_res, n_ref = len(res_pad), len(ref_pad)
    bx = max([o for _, _, o in pairs] + list(res_pad) + list(ref_pad)) + 2
    res = np.zeros((3, 2 * n_ref, n_res * bx), bool)
    ref = np.zeros_like(res)
    for j, i, o in pairs:
        res[1, 2 * (j - 1), (i - 1) * bx:(i - 1) * bx + o] = True
        ref[1, 2 * (j - 1), (i - 1) * bx:(i - 1) * bx + o] = True
    for i in range(1, n_res + 1):
        rows = [j for j, ii, _ in pairs if ii == i]
        res[0, 0:2 * (max(rows) - 1) + 1, (i - 1) * bx] = True                    # the joint, from row 0: numbering by column
        res[0, 0, (i - 1) * bx:(i - 1) * bx + 1 + res_pad[i - 1]] = True
    for j in range(1, n_ref + 1):
        cols = [i for jj, i, _ in pairs if jj == j]
        ref[2, 2 * (j - 1), (min(cols) - 1) * bx:(max(cols) - 1) * bx + 1 + ref_pad[j - 1]] = True
    return res, ref


LAYOUTS = [
    # reference 1 overlaps results {1, 2, 3}, reference 2 overlaps {1, 2}: the smaller set goes first and takes result 1
    ("set_size_decides", [(1, 1, 6), (1, 2, 5), (1, 3, 1), (2, 1, 4), (2, 2, 3)], [0, 0, 6], [0, 2]),
    # reference 3's single candidate takes result 3 first: reference 1's set {2, 3, 4} shrinks to two and ties with reference 2's
    ("used_candidate_shrinks_a_set", [(1, 2, 5), (1, 3, 4), (1, 4, 1), (2, 1, 1), (2, 2, 6), (3, 3, 6)], [6, 0, 0, 6], [0, 2, 3]),
    ("equal_overlaps_lowest_id_first", [(1, 1, 5), (1, 2, 5)], [0, 0], [0]),
    ("equal_set_sizes_keep_id_order", [(1, 1, 4), (1, 2, 4), (2, 1, 4), (2, 2, 4)], [0, 0], [0, 0]),
    ("largest_overlap_fails_next_passes", [(1, 1, 6), (1, 2, 5)], [12, 0], [0]),
    ("used_single_candidate_stays_unmatched", [(1, 1, 8), (2, 1, 8), (3, 1, 1), (3, 2, 7)], [0, 0], [0, 0, 0]),
    # references 1 and 2 take results 1 and 2; reference 3's set {1, 2} is empty before it is looked at
    ("set_emptied_by_earlier_matches", [(1, 1, 8), (2, 2, 8), (3, 1, 2), (3, 2, 2)], [0, 0], [0, 0, 0]),
    # two waiting references want the same result object most; the second keeps its second choice
    ("contested_by_two_waiting_sets", [(1, 1, 7), (1, 2, 2), (2, 1, 6), (2, 3, 5)], [0, 4, 0], [0, 0]),
]


# ------------------------------------------------------------------------------------------------- records
def rows_of(labeled_res, labeled_ref, mapping):
    """[(ref first voxel, res first voxel, intersection, ref size, res size)] in the mapping's order."""
    out = []
    for ref_id, (res_id, score) in mapping.items():
        a, b = labeled_ref == ref_id, labeled_res == res_id
        inter, sa, sb = int(np.count_nonzero(a & b)), int(np.count_nonzero(a)), int(np.count_nonzero(b))
        assert float(score) == 2.0 * inter / float(sa + sb)
        out.append((int(np.flatnonzero(a)[0]), int(np.flatnonzero(b)[0]), inter, sa, sb))
    return out


def write_npz(path, arrays):
    """np.load-able, and the same bytes on every run: stored entries with a fixed date."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ak = _import_reference()
    cases = list(random_pairs())
    for name, pairs, res_pad, ref_pad in LAYOUTS:
        res, ref = layout(pairs, res_pad, ref_pad)
        lres, n_res = ndi.label(res)
        lref, n_ref = ndi.label(ref)
        assert (n_res, n_ref) == (len(res_pad), len(ref_pad)), name
        for j, i, o in pairs:                                                   # numbered as the table says
            assert np.count_nonzero((lref == j) & (lres == i)) == o, (name, j, i)
        assert np.count_nonzero((lres > 0) & (lref > 0)) == sum(o for _, _, o in pairs), name
        cases.append((name, res, ref))
    shapes, bits, bit_off, counts, match_rows, match_off = [], [], [0], [], [], [0]
    for name, res, ref in cases:
        assert res.shape == ref.shape and res.ndim == 3
        shapes.append(res.shape)
        for v in (res, ref):
            bits.append(np.packbits(v.ravel()))
            bit_off.append(bit_off[-1] + len(bits[-1]))
        line = [name]
        for k, thresh in enumerate(THRESHOLDS):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                lres, lref, n_res, n_ref, mapping = ak.distinct_binary_object_correspondences(
                    res.astype(np.uint8), ref.astype(np.uint8), thresh)
            if k == 0:
                counts.append((n_res, n_ref))
            assert counts[-1] == (n_res, n_ref)
            rows = rows_of(lres, lref, mapping)
            match_rows += rows
            match_off.append(len(match_rows))
            line.append(len(rows))
        print(line, counts[-1])
    out = {"names": np.array(json.dumps([c[0] for c in cases])), "thresholds": np.array(THRESHOLDS, np.float64),
           "shapes": np.array(shapes, np.int32), "bits": np.concatenate(bits), "bit_offsets": np.array(bit_off, np.int64),
           "counts": np.array(counts, np.int32), "matches": np.array(match_rows, np.int64).reshape(-1, 5),
           "match_offsets": np.array(match_off, np.int64)}
    path = os.path.join(HERE, "ref_detection.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
