"""Spatial-guide fixtures pinned on the REFERENCE ITSELF (build container only): `create_gaussian_distribution_v2` of the
reference's utils/array_kits.py -- the numpy twin of image_ops.create_spatial_guide_2d, which the guided LiTS pipeline renders
per sample (DataLoader/Liver/input_pipeline_g.py:382-412) -- on seeded inputs, written to tests/golden/ref_sp_guide.npz.

    python tests/golden/make_guide_fixtures.py         # needs the reference checkout; rewrites ref_sp_guide.npz

array_kits imports skimage and medpy at module level for functions the guide does not use; empty stand-ins are put into
sys.modules first so that the module imports with numpy and scipy alone.  The stddevs are floored at 1.0 here (the render
floor of the pipeline), so a kernel call with min_std = 1.0 and crop == output size must reproduce g / 2 + 0.5.
tests/test_lits_guide_host.py (numpy restatement) and tests/test_gpu_lits_guide.py (unetk_lits_spatial_guide) read the file."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# (H, W, number of objects): square / non-square / one object / many objects / a single pixel
CASES = [(32, 32, 1), (24, 40, 3), (17, 9, 5), (48, 48, 15), (1, 1, 2), (7, 31, 40)]


def _import_array_kits():
    for name in ("skimage", "skimage.feature", "skimage._shared", "skimage._shared.utils", "medpy", "medpy.metric"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].feature = sys.modules["skimage.feature"]
    sys.modules["skimage"]._shared = sys.modules["skimage._shared"]
    sys.modules["skimage._shared"].utils = sys.modules["skimage._shared.utils"]
    sys.modules["medpy"].metric = sys.modules["medpy.metric"]
    sys.path.insert(0, os.path.join(REF, "utils"))
    import array_kits
    return array_kits


def main():
    ak = _import_array_kits()
    rng = np.random.RandomState(2024)
    out = {}
    for i, (h, w, k) in enumerate(CASES):
        # centres inside and around the crop (off-crop centres leave tails), stddevs from sub-pixel (floored) to wide
        centers = np.stack([rng.uniform(-3, h + 3, k), rng.uniform(-3, w + 3, k)], axis=1).astype(np.float32)
        stddevs = np.maximum(rng.uniform(0.0, max(h, w) / 2.0, (k, 2)), 1.0).astype(np.float32)
        g = ak.create_gaussian_distribution_v2([h, w], centers, stddevs, "ij")
        out["case{}_centers".format(i)] = centers
        out["case{}_stddevs".format(i)] = stddevs
        out["case{}_guide".format(i)] = np.asarray(g, np.float32)
    out["shapes"] = np.array(CASES, dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "ref_sp_guide.npz"), **out)
    print("wrote ref_sp_guide.npz:", ", ".join("{}x{} ({} objects)".format(*c) for c in CASES))


if __name__ == "__main__":
    main()
