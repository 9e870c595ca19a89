"""GLCM context fixtures pinned on the REFERENCE ITSELF (build container only): the per-slice co-occurrence texture rows of
the reference's DataLoader/Liver/extract.py -- `dump_glcm_feature_for_train` and `dump_glcm_feature_for_eval` with
average_num=3, norm_levels=True, as `run_dump_glcm_feature_for_{train,eval}` call them -- on small synthetic cases, written
to tests/golden/ref_glcm_feature.npz (volumes, labels, the meta records as JSON, and the rows of both modes).

    python tests/golden/make_glcm_fixtures.py         # needs the reference checkout; rewrites ref_glcm_feature.npz

extract.py imports cv2, SimpleITK, nibabel and (through utils/array_kits) skimage and medpy at module level; empty stand-ins
are put into sys.modules first.  scikit-image is not installed, so `skimage.feature.greycomatrix` is a plain-numpy
restatement of its counting rule (levels x levels x distances x angles; offset (round(sin(a) d), round(cos(a) d)); every pixel
whose partner lies inside the image counts once; symmetric adds the transpose; normed divides by the sum, a zero sum taken
as 1) and `skutils.assert_nD` a no-op.  The golden therefore pins patch choice, smoothing, zoom, the property formulas, the
scaling, the averaging and the row layout on the reference's own code; the counting rule is pinned by the brute-force loop of
tests/test_gpu_glcm.py.  `nii_kits.read_lits` and `json.load` are monkeypatched to serve the synthetic cases and their meta
records (the reference opens its own prepare/meta.json, which exists).
tests/test_glcm_host.py (numpy restatement) and tests/test_gpu_glcm.py (unetk_glcm_features) read the file."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SHAPE = (8, 48, 48)


def _meta(pid, labels):
    """The fields of a meta.json record the glcm dumps read, derived as the exporter derives them: 18-connected 3-D tumour
    components, and per slice of each its area and tight box (y1, x1, y2, x2), grouped by slice."""
    tumors, _ = ndi.label(labels == 2, ndi.generate_binary_structure(3, connectivity=2))
    slices = ndi.find_objects(tumors)
    objects = [[z.start, y.start, x.start, z.stop, y.stop, x.stop] for z, y, x in slices]
    by_z = {z: [] for z in range(labels.shape[0])}
    for tid, sli in enumerate(slices):
        region = labels[sli] == 2
        for k in range(region.shape[0]):
            ys, xs = np.nonzero(region[k])
            box = [int(ys.min()) + objects[tid][1], int(xs.min()) + objects[tid][2],
                   int(ys.max()) + 1 + objects[tid][1], int(xs.max()) + 1 + objects[tid][2]]
            by_z[objects[tid][0] + k].append((tid, int(region[k].sum()), box))
    index = [z for z in by_z if by_z[z]]
    from_to, areas, boxes, tids = [0], [], [], []
    for z in index:
        from_to.append(from_to[-1] + len(by_z[z]))
        for tid, area, box in by_z[z]:
            tids.append(tid)
            areas.append(area)
            boxes.append(box)
    return {"PID": pid, "size": list(labels.shape), "tumors": objects, "tumor_slices_index": index,
            "tumor_slices_from_to": from_to, "tumor_slices_areas": areas, "tumor_slices": boxes, "tumor_slices_tid": tids}


def make_cases():
    """3 cases.  0: one tumour alone on its first slices (the zoom loop runs twice), a second one overlapping it in z (two
    tumours on a slice: one zoom round; an eval counter of 2), a 9-pixel tumour alone on the last slice (skipped: the row
    stays zero).  1: three tumours on a slice (no zoom), one of them a box of constant HU.  2: a tumour one pixel wide and a
    tumour in the image corner."""
    rng = np.random.RandomState(2024)
    cases = []
    for i in range(3):
        vol = (ndi.gaussian_filter(rng.normal(size=SHAPE), (0.5, 1.5, 1.5)) * 400. + 60.).astype(np.int16)
        vol[rng.rand(*SHAPE) < 0.02] = rng.choice([-400, -250, 300, 500])               # values at and beyond the window
        lab = np.zeros(SHAPE, np.uint8)
        lab[:, 2:46, 2:46] = 1
        if i == 0:
            lab[1:5, 5:15, 5:17] = 2
            lab[3:7, 25:35, 20:30] = 2
            lab[7, 40:43, 40:43] = 2
        elif i == 1:
            lab[2:4, 4:12, 4:14] = 2
            lab[2:4, 20:27, 8:15] = 2
            lab[2:5, 30:40, 30:42] = 2
            vol[2:5, 30:40, 30:42] = 120
        else:
            lab[1:3, 4:28, 10:11] = 2
            lab[4:7, 0:8, 40:48] = 2
        cases.append((vol, lab, _meta(i, lab)))
    return cases


def greycomatrix(image, distances, angles, levels=256, symmetric=False, normed=False):
    image = np.ascontiguousarray(image)
    rows, cols = image.shape
    P = np.zeros((levels, levels, len(distances), len(angles)), dtype=np.uint32)
    for di, d in enumerate(distances):
        for ai, a in enumerate(angles):
            dr, dc = int(round(np.sin(a) * d)), int(round(np.cos(a) * d))
            r0, r1 = max(0, -dr), min(rows, rows - dr)
            c0, c1 = max(0, -dc), min(cols, cols - dc)
            if r1 <= r0 or c1 <= c0:
                continue
            src = image[r0:r1, c0:c1].reshape(-1)
            dst = image[r0 + dr:r1 + dr, c0 + dc:c1 + dc].reshape(-1)
            np.add.at(P[:, :, di, ai], (src, dst), 1)
    if symmetric:
        P = P + np.transpose(P, (1, 0, 2, 3))
    if normed:
        P = P.astype(np.float64)
        sums = np.apply_over_axes(np.sum, P, axes=(0, 1))
        sums[sums == 0] = 1
        P /= sums
    return P


def _import_extract():
    for name in ("cv2", "SimpleITK", "nibabel", "skimage", "skimage.feature", "skimage._shared", "skimage._shared.utils",
                 "medpy", "medpy.metric"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].feature = sys.modules["skimage.feature"]
    sys.modules["skimage"]._shared = sys.modules["skimage._shared"]
    sys.modules["skimage._shared"].utils = sys.modules["skimage._shared.utils"]
    sys.modules["medpy"].metric = sys.modules["medpy.metric"]
    sys.modules["skimage.feature"].greycomatrix = greycomatrix
    sys.modules["skimage._shared.utils"].assert_nD = lambda *a, **k: None
    sys.path.insert(0, REF)
    from DataLoader.Liver import extract
    return extract


def main():
    extract = _import_extract()
    cases = make_cases()
    arrays = {i: c for i, c in enumerate(cases)}

    def read_lits(num, obj, file_name, only_header=False):
        vol, lab, _ = arrays[int(num)]
        return None, (vol if obj == "vol" else lab)

    extract.nii_kits.read_lits = read_lits
    extract.json.load = lambda f: [json.loads(json.dumps(m)) for _, _, m in cases]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "nii")
        os.makedirs(src)
        for i in arrays:
            for stem in ("volume", "segmentation"):
                open(os.path.join(src, "{}-{}.nii".format(stem, i)), "wb").close()
        dst = os.path.join(tmp, "feat")
        extract.dump_glcm_feature_for_train(src, dst, average_num=3, norm_levels=True)
        extract.dump_glcm_feature_for_eval(src, dst, average_num=3, norm_levels=True)
        for i, (vol, lab, meta) in arrays.items():
            out["vol_%d" % i], out["lab_%d" % i] = vol, lab
            out["meta_%d" % i] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
            for mode in ("train", "eval"):
                out["%s_%d" % (mode, i)] = np.load(os.path.join(dst, mode, "%03d.npy" % i))
    path = os.path.join(HERE, "ref_glcm_feature.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
