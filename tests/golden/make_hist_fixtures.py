"""Context-guide fixtures pinned on the REFERENCE ITSELF (build container only): the per-slice histogram features of the
reference's DataLoader/Liver/extract.py -- `dump_hist_feature_v2` (mode "eval": tumour pixels of each 18-connected tumour's
middle slice, tiled over its z-extent) and `dump_hist_feature` (mode "train": the slice's own tumour pixels), both with 100
bins over (-200, 250) as `run_dump_hist_feature` calls them -- on small synthetic cases, written to
tests/golden/ref_hist_feature.npz.

    python tests/golden/make_hist_fixtures.py         # needs the reference checkout; rewrites ref_hist_feature.npz

extract.py imports cv2, SimpleITK and nibabel at module level, and utils/array_kits skimage and medpy, for functions the
histograms do not use; empty stand-ins are put into sys.modules first.  `nii_kits.read_lits` is monkeypatched to return
the synthetic arrays, and the `volume-*.nii` glob finds empty placeholder files in a temporary directory.
tests/test_lits_context_host.py (numpy restatement) and tests/test_gpu_lits_context.py (unetk_slice_hist) read the file."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SHAPE = (12, 40, 48)
XRNG = (-200, 250)


def make_cases():
    """4 cases: HU values outside the range and on bin edges, slices without liver, liver slices without tumour, two
    tumours with overlapping z-extents, tumours joined only through an edge (one 18-connected component, two
    6-connected ones), tumours touching only at a corner (two components), and a case of many random blobs."""
    rng = np.random.RandomState(77)
    d, h, w = SHAPE
    edges = np.linspace(XRNG[0], XRNG[1], 101)
    on_edge = edges[::2].astype(np.int16)                                       # every even edge is an integer
    cases = []
    for i in range(4):
        vol = rng.randint(-320, 380, size=SHAPE).astype(np.int16)
        pick = rng.rand(*SHAPE) < 0.15
        vol[pick] = rng.choice(np.concatenate([on_edge, [-201, 251, 250, -200]]), size=int(pick.sum()))
        lab = np.zeros(SHAPE, np.uint8)
        lab[2:d - 2, 5:35, 6:42] = 1                                            # no liver on slices 0, 1, d-2, d-1
        if i == 0:            # two tumours, z-extents [3, 8) and [5, 10) overlapping
            lab[3:8, 8:14, 8:16] = 2
            lab[5:10, 20:30, 25:33] = 2
            lab[6, 22, 27] = 1
        elif i == 1:          # joined only through in-plane / through-plane edges
            lab[4:7, 10:14, 10:14] = 2
            lab[5:7, 14:17, 14:18] = 2                                          # (y 13 -> 14, x 13 -> 14): an edge
            lab[7:9, 24:27, 30:33] = 2
            lab[9:10, 27:29, 30:33] = 2                                         # (z 8 -> 9, y 26 -> 27): an edge
        elif i == 2:          # touching only at corners: separate components
            lab[3:6, 10:13, 10:13] = 2
            lab[6:8, 13:16, 13:16] = 2                                          # (5, 12, 12) -> (6, 13, 13): a corner
            lab[8, 20, 20] = 2
            lab[9, 21, 21] = 2
        else:                 # many random blobs, some outside the liver box
            for _ in range(12):
                z, y, x = rng.randint(0, d - 3), rng.randint(0, h - 5), rng.randint(0, w - 5)
                lab[z:z + rng.randint(1, 4), y:y + rng.randint(1, 6), x:x + rng.randint(1, 6)] = 2
        cases.append((vol, lab))
    return cases


def _import_extract():
    for name in ("cv2", "SimpleITK", "nibabel", "skimage", "skimage.feature", "skimage._shared", "skimage._shared.utils",
                 "medpy", "medpy.metric"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].feature = sys.modules["skimage.feature"]
    sys.modules["skimage"]._shared = sys.modules["skimage._shared"]
    sys.modules["skimage._shared"].utils = sys.modules["skimage._shared.utils"]
    sys.modules["medpy"].metric = sys.modules["medpy.metric"]
    sys.path.insert(0, REF)
    from DataLoader.Liver import extract
    return extract


def main():
    extract = _import_extract()
    cases = make_cases()
    arrays = {int(i): c for i, c in enumerate(cases)}

    def read_lits(num, obj, file_name, only_header=False):
        vol, lab = arrays[int(num)]
        return None, (vol if obj == "vol" else lab)

    extract.nii_kits.read_lits = read_lits
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "nii")
        os.makedirs(src)
        for i in arrays:
            for stem in ("volume", "segmentation"):
                open(os.path.join(src, "{}-{}.nii".format(stem, i)), "wb").close()
        dst = os.path.join(tmp, "feat")
        extract.dump_hist_feature(src, dst, mode="train", bins=100, xrng=XRNG, number=-1)
        extract.dump_hist_feature_v2(src, dst, mode="eval", bins=100, xrng=XRNG, number=-1)
        for i, (vol, lab) in arrays.items():
            out["vol_%d" % i], out["lab_%d" % i] = vol, lab
            for mode in ("train", "eval"):
                out["%s_%d" % (mode, i)] = np.load(os.path.join(dst, mode, "%03d.npy" % i))
    np.savez_compressed(os.path.join(HERE, "ref_hist_feature.npz"), **out)
    print("wrote", os.path.join(HERE, "ref_hist_feature.npz"), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
