"""NIfTI -> training-set export of LiTS -- host-side mirror of the reference's DataLoader/Liver/extract.py:61-213
(`process_case`, `nii_3d_to_png`): per case the HU volume is clipped to [-200, 250], shifted and scaled by 64 into 16-bit
PNG slices `<out>/volume-<PID>/<z:03d>_im.png`, the labels x 64 into `<z:03d>_lb.png`, and `meta.json` receives the
record `data/lits.py` consumes (size, spacing, liver box, 3-D tumour components with robust centre / spread, and the same
per slice).  Pure host code on this package's NIfTI and PNG codecs (no nibabel / SimpleITK in this image)."""
import json
from pathlib import Path

import numpy as np
import scipy.ndimage as ndi

from ..utils import array_kits
from . import nii_kits
from .lits import GRAY_MAX, GRAY_MIN, IM_SCALE, LB_SCALE, png_encode


def process_case(vol_case, dst_path, only_meta=False):
    """extract.py:61-189 for one `volume-<PID>.nii[.gz]` (its labels next to it as `segmentation-<PID>`)."""
    vol_case, dst_path = Path(vol_case), Path(dst_path)
    stem = vol_case.name.split(".")[0]
    pid = int(stem.split("-")[-1])
    vh, volume = nii_kits.read_nii(vol_case, out_dtype=np.int16, special=28 <= pid < 48)
    volume = ((np.clip(volume, GRAY_MIN, GRAY_MAX) - GRAY_MIN) * IM_SCALE).astype(np.uint16)
    lab_case = vol_case.parent / vol_case.name.replace("volume", "segmentation")
    _, labels = nii_kits.read_nii(lab_case, out_dtype=np.uint8, special=28 <= pid < 52)
    assert volume.shape == labels.shape, "Vol{} vs Lab{}".format(volume.shape, labels.shape)

    b = array_kits.extract_region(labels).tolist()                   # (x1, y1, z1, x2, y2, z2) inclusive
    bbox = [int(b[2]), int(b[1]), int(b[0]), int(b[5]) + 1, int(b[4]) + 1, int(b[3]) + 1]

    disc3 = ndi.generate_binary_structure(3, connectivity=2)
    tumors, _ = ndi.label(labels == 2, disc3)
    slices = ndi.find_objects(tumors)
    objects = [[z.start, y.start, x.start, z.stop, y.stop, x.stop] for z, y, x in slices]
    all_centers, all_stddevs, tumor_areas = [], [], []
    per_tumor = {i: {"centers": [], "stddevs": [], "areas": [], "slices": []} for i in range(len(slices))}
    z_rev = {i: {"tid": [], "rid": []} for i in range(volume.shape[0])}
    for j, sli in enumerate(slices):
        # NB labels[sli] == 2 of the bounding box, as the reference: voxels of OTHER tumours inside the box count too
        region = labels[sli] == 2
        center, stddev = array_kits.compute_robust_moments(region, indexing="ij", min_std=0.)
        center = center + np.array(objects[j][:3], np.float32)
        all_centers.append(center.tolist())
        all_stddevs.append([round(float(x), 3) for x in stddev])
        tumor_areas.append(int(np.count_nonzero(region)))
        for k in range(region.shape[0]):
            patch = region[k]
            c2, s2 = array_kits.compute_robust_moments(patch, indexing="ij", min_std=0.)
            c2 = c2 + np.array(objects[j][1:3], np.float32)
            per_tumor[j]["centers"].append(c2.tolist())
            per_tumor[j]["stddevs"].append([round(float(x), 3) for x in s2])
            per_tumor[j]["areas"].append(int(np.count_nonzero(patch)))
            x1, y1, x2, y2 = [int(v) for v in array_kits.bbox_from_mask(patch, mask_values=1).tolist()]
            per_tumor[j]["slices"].append([y1 + objects[j][1], x1 + objects[j][2], y2 + 1 + objects[j][1], x2 + 1 + objects[j][2]])
            z_rev[objects[j][0] + k]["tid"].append(j)
            z_rev[objects[j][0] + k]["rid"].append(k)

    index = [j for j in z_rev if len(z_rev[j]["tid"]) > 0]
    from_to, centers, stddevs, areas, boxes, tids = [0], [], [], [], [], []
    for j in index:
        from_to.append(from_to[-1] + len(z_rev[j]["tid"]))
        for tid, rid in zip(z_rev[j]["tid"], z_rev[j]["rid"]):
            centers.append(per_tumor[tid]["centers"][rid])
            stddevs.append(per_tumor[tid]["stddevs"][rid])
            areas.append(per_tumor[tid]["areas"][rid])
            boxes.append(per_tumor[tid]["slices"][rid])
            tids.append(tid)

    meta = {"PID": pid, "vol_case": str(vol_case), "lab_case": str(lab_case),
            "size": [int(x) for x in vh.get_data_shape()[::-1]], "spacing": [float(x) for x in vh.get_zooms()[::-1]],
            "bbox": bbox, "tumors": objects, "tumor_areas": tumor_areas, "tumor_centers": all_centers,
            "tumor_stddevs": all_stddevs, "tumor_slices_from_to": from_to, "tumor_slices": boxes, "tumor_slices_index": index,
            "tumor_slices_centers": centers, "tumor_slices_stddevs": stddevs, "tumor_slices_areas": areas,
            "tumor_slices_tid": tids}
    if not only_meta:
        dst_dir = dst_path / stem
        dst_dir.mkdir(parents=True, exist_ok=True)
        for j, (img, lab) in enumerate(zip(volume, labels * LB_SCALE)):
            (dst_dir / "{:03d}_im.png".format(j)).write_bytes(png_encode(np.ascontiguousarray(img)))
            (dst_dir / "{:03d}_lb.png".format(j)).write_bytes(png_encode(np.ascontiguousarray(lab.astype(np.uint8))))
    return meta


def nii_3d_to_png(in_path, out_path, only_meta=False):
    """extract.py:192-213: every volume-*.nii[.gz] of in_path -> out_path/volume-<PID>/*.png + out_path/meta.json."""
    src, dst = Path(in_path), Path(out_path)
    dst.mkdir(parents=True, exist_ok=True)
    files = sorted(list(src.glob("volume-*.nii")) + list(src.glob("volume-*.nii.gz")),
                   key=lambda x: int(x.name.split(".")[0].split("-")[-1]))
    metas = sorted((process_case(f, dst, only_meta) for f in files), key=lambda m: m["PID"])
    with (dst / "meta.json").open("w") as f:
        json.dump(metas, f)
    return metas


HIST_RANGE = (-200, 250)        # extract.py's (GRAY_MIN + 50, GRAY_MAX - 50) of its own GRAY_MIN / GRAY_MAX = -250 / 300


def dump_hist_feature(in_path, out_path, mode, bins=100, xrng=HIST_RANGE, device=None):
    """extract.py:237-375 (`dump_hist_feature` for mode "train", `dump_hist_feature_v2` for mode "eval", as
    `run_dump_hist_feature` calls them): for every volume-<PID>.nii[.gz] of in_path (labels next to it as segmentation-<PID>)
    the per-slice histogram rows float32 [depth, 2 bins] -> <out_path>/hist/<mode>/<PID:03d>.npy, the files the guided
    pipeline reads with --use_context --context_list hist 200.  The rows are computed on the device (ops.slice_hist,
    bit-identical to the reference's numpy loop); reading the NIfTI files stays on the host.  Returns the written paths."""
    import torch

    from .. import ops
    if mode not in ("train", "eval"):
        raise ValueError("mode must be `train` or `eval`, got {}".format(mode))
    device = device or torch.device("cuda", torch.cuda.current_device())
    src = Path(in_path)
    dst = Path(out_path) / "hist" / mode
    dst.mkdir(parents=True, exist_ok=True)
    files = sorted(list(src.glob("volume-*.nii")) + list(src.glob("volume-*.nii.gz")),
                   key=lambda x: int(x.name.split(".")[0].split("-")[-1]))
    written = []
    for vol_case in files:
        pid = int(vol_case.name.split(".")[0].split("-")[-1])
        _, volume = nii_kits.read_lits(pid, "vol", vol_case)
        _, labels = nii_kits.read_lits(pid, "lab", vol_case.parent / vol_case.name.replace("volume", "segmentation"))
        assert volume.shape == labels.shape, "Vol{} vs Lab{}".format(volume.shape, labels.shape)
        vol_d = torch.from_numpy(np.ascontiguousarray(volume, dtype=np.int16)).to(device)
        lab_d = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)).to(device)
        rows = ops.slice_hist(vol_d, lab_d, mode, bins, xrng).cpu().numpy()
        out = dst / "{:03d}.npy".format(pid)
        np.save(out, rows)
        written.append(out)
    return written


GLCM_GRAY = (-250, 300)         # extract.py's own GRAY_MIN / GRAY_MAX: the window the uint8 levels of the glcm patches come from
GLCM_FILTER_SIZE = 20           # run_dump_glcm_feature_for_{train,eval}: tumours on a slice smaller than this are skipped
GLCM_AVERAGE_NUM = 3            # ... and at least this many patches are averaged per row


def _glcm_patch(image, loop):
    """The patch of zoom loop `loop` (0 = plain) as the reference makes it: ndi.zoom(order=1) by 1 + 0.1 loop, then
    ndi.gaussian_filter(., 0.5) ON THE uint8 ARRAY -- scipy rounds back to uint8 after each axis, which the levels depend on."""
    import warnings
    if loop > 0:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            image = ndi.zoom(image, (1. + loop * .1,) * 2, order=1)
    return np.ascontiguousarray(ndi.gaussian_filter(image, 0.5))


def glcm_patches(volume, case, mode, filter_size=GLCM_FILTER_SIZE, average_num=GLCM_AVERAGE_NUM):
    """The smoothed uint8 patches of one case and how the rows are made of them (extract.py:465-512 for "train", :607-643
    for "eval"): (patches, groups), groups = [(z1, z2, [patch indices])] -- the float64 mean of a group's feature vectors
    goes to rows [z1, z2) (train: one slice, assigned; eval: a tumour's z-extent, accumulated and counted).  volume: uint8
    [depth, H, W]; case: its meta.json record."""
    from .lits import _maybe_json
    index = list(_maybe_json(case["tumor_slices_index"]))
    from_to = _maybe_json(case["tumor_slices_from_to"])
    areas = _maybe_json(case["tumor_slices_areas"])
    boxes = _maybe_json(case["tumor_slices"])
    patches, groups = [], []

    def add(k, j, loop):
        y1, x1, y2, x2 = boxes[j]
        patches.append(_glcm_patch(volume[k, y1:y2, x1:x2], loop))
        return len(patches) - 1

    if mode == "train":
        for k in range(volume.shape[0]):
            if k not in index:
                continue
            ind = index.index(k)
            js = [j for j in range(from_to[ind], from_to[ind + 1]) if areas[j] >= filter_size]
            if not js:
                continue                      # every tumour of the slice is below filter_size: the row stays zero
            members = [add(k, j, 0) for j in js]
            loop = 1
            while len(members) < average_num:
                members += [add(k, j, loop) for j in js]
                loop += 1
            groups.append((k, k + 1, members))
        return patches, groups
    tids = _maybe_json(case["tumor_slices_tid"])
    for tid, (z1, _, _, z2, _, _) in enumerate(_maybe_json(case["tumors"])):
        middle = (z2 - z1 - 1) // 2 + z1
        ind = index.index(middle)
        for j in range(from_to[ind], from_to[ind + 1]):
            if tids[j] == tid:
                if areas[j] >= filter_size:   # only the first record of the tumour on its middle slice is looked at
                    groups.append((z1, z2, [add(middle, j, loop) for loop in range(average_num)]))
                break
    return patches, groups


def glcm_rows(feats, groups, depth, mode):
    """float32 [depth, F] rows from the float64 [n, F] feature vectors of glcm_patches' patches, in the reference's dtypes:
    train rows are the float64 mean stored as float32; eval rows accumulate the float64 means into float32 and are divided
    by max(count, 1) in float64."""
    width = feats.shape[1] if feats.ndim == 2 else 0
    rows = np.zeros((depth, width), dtype=np.float32)
    counter = np.zeros((depth,), dtype=np.int32)
    for z1, z2, members in groups:
        mean = np.mean([feats[m] for m in members], axis=0)
        if mode == "train":
            rows[z1] = mean
        else:
            rows[z1:z2] += np.tile(mean[None], (z2 - z1, 1))
            counter[z1:z2] += 1
    if mode != "train":
        rows /= np.clip(counter, 1, np.inf)[:, None]
    return rows


def dump_glcm_feature(in_path, out_path, mode, meta, device=None):
    """extract.py:377-661 (`dump_glcm_feature_for_train` / `dump_glcm_feature_for_eval` as run_dump_glcm_feature_for_* call
    them: all 8 properties, distances 1 2 3, angles 0 45 90 135, filter_size 20, average_num 3, norm_levels): for every
    volume-<PID>.nii[.gz] of in_path the float32 [depth, 96] rows -> <out_path>/glcm/<mode>/<PID:03d>.npy, the files the
    guided pipeline reads with --use_context --glcm --context_list ... glcm 96.  meta: the meta.json records (a list, or the
    path of the file).  Cutting, zooming and smoothing the tumour boxes stays on the host (scipy's own uint8 rounding is part
    of the result); every patch of a case goes to the device in ONE ops.glcm_features call.  Returns the written paths."""
    from .. import ops
    if mode not in ("train", "eval"):
        raise ValueError("mode must be `train` or `eval`, got {}".format(mode))
    if isinstance(meta, (str, Path)):
        with Path(meta).open() as f:
            meta = json.load(f)
    meta = {int(case["PID"]): case for case in meta}
    src = Path(in_path)
    dst = Path(out_path) / "glcm" / mode
    dst.mkdir(parents=True, exist_ok=True)
    files = sorted(list(src.glob("volume-*.nii")) + list(src.glob("volume-*.nii.gz")),
                   key=lambda x: int(x.name.split(".")[0].split("-")[-1]))
    width = 8 * len(ops.glcm_offsets())
    written = []
    for vol_case in files:
        pid = int(vol_case.name.split(".")[0].split("-")[-1])
        if pid not in meta:
            raise KeyError("case {} has no record in the meta file".format(pid))
        _, volume = nii_kits.read_lits(pid, "vol", vol_case)
        lo, hi = GLCM_GRAY
        volume = ((np.clip(volume, lo, hi) - lo) * (255. / (hi - lo))).astype(np.uint8)
        patches, groups = glcm_patches(volume, meta[pid], mode)
        feats = ops.glcm_features(patches, norm_levels=True, device=device) if patches else np.zeros((0, width))
        out = dst / "{:03d}.npy".format(pid)
        np.save(out, glcm_rows(feats.reshape(-1, width), groups, volume.shape[0], mode))
        written.append(out)
    return written


def simulate_user_prior(meta):
    """extract.py:664-717 `simulate_user_prior` on a list of meta.json records: for every 3-D tumour (z1, y1, x1, z2, y2,
    x2) its middle slice (z2 - z1 - 1) // 2 + z1 receives {"z": [z1, z2], "center", "stddev"} of that tumour's 2-D record
    on that slice.  Keys: string PIDs, then string slice ids (what json.dump makes of the reference's int keys)."""
    from .lits import _maybe_json
    prior = {}
    for case in meta:
        tumors = _maybe_json(case["tumors"])
        index = _maybe_json(case["tumor_slices_index"])
        from_to = _maybe_json(case["tumor_slices_from_to"])
        tids = _maybe_json(case["tumor_slices_tid"])
        centers = _maybe_json(case["tumor_slices_centers"])
        stddevs = _maybe_json(case["tumor_slices_stddevs"])
        slices = {}
        for tid, (z1, _, _, z2, _, _) in enumerate(tumors):
            middle = (z2 - z1 - 1) // 2 + z1
            ind = index.index(middle)
            for j in range(from_to[ind], from_to[ind + 1]):
                if tids[j] == tid:
                    slices.setdefault(str(middle), []).append({"z": [z1, z2], "center": centers[j], "stddev": stddevs[j]})
        prior[str(case["PID"])] = slices
    return prior


def write_user_prior(lits_root):
    """<lits_root>/meta.json -> <lits_root>/prior.json (simulate_user_prior); returns the path."""
    root = Path(lits_root)
    with (root / "meta.json").open() as f:
        meta = json.load(f)
    out = root / "prior.json"
    with out.open("w") as f:
        json.dump(simulate_user_prior(meta), f)
    return out


NEG_DIR = "neg3d"              # <lits_root>/neg3d/neg-<PID>.npz: what liver_3d --hard_neg_from reads
NEG_MIN_SIZE = 6               # load_neg drops components of size <= 5 (input_pipeline_3d.py:216)


def save_neg(path, mask, slice_counts, kept, components):
    """One case's false-positive mask as `mine_false_positives` writes it: `bits` = np.packbits of the 0/1 mask in (z, y, x)
    order, `shape`, `slice_counts` int64 [depth], `kept` and `components`."""
    mask = np.ascontiguousarray(np.asarray(mask) != 0)
    np.savez(path, bits=np.packbits(mask.reshape(-1)), shape=np.asarray(mask.shape, dtype=np.int64),
             slice_counts=np.asarray(slice_counts, dtype=np.int64), kept=np.int64(kept), components=np.int64(components))


def load_neg(path):
    """dict(bits uint8 [ceil(n / 8)], shape (d, h, w), slice_counts int64 [d], kept, components) of a neg-<PID>.npz; a file that
    does not hold these, or whose parts disagree in size, is an error naming it."""
    try:
        with np.load(path) as f:
            rec = dict(bits=np.ascontiguousarray(f["bits"], dtype=np.uint8), shape=tuple(int(v) for v in f["shape"]),
                       slice_counts=np.asarray(f["slice_counts"], dtype=np.int64), kept=int(f["kept"]),
                       components=int(f["components"]))
    except (KeyError, ValueError, OSError) as e:
        if isinstance(e, FileNotFoundError):
            raise
        raise ValueError("{}: not a neg-<PID>.npz of `extract neg3d`: {}".format(path, e))
    n = int(np.prod(rec["shape"])) if len(rec["shape"]) == 3 else -1
    if n < 0 or rec["bits"].shape != ((n + 7) // 8,) or rec["slice_counts"].shape != (rec["shape"][0],):
        raise ValueError("{}: bits / slice_counts do not fit the shape {}".format(path, rec["shape"]))
    return rec


def unpack_neg(rec):
    """The 0/1 uint8 mask [d, h, w] of a load_neg record (host)."""
    n = int(np.prod(rec["shape"]))
    return np.unpackbits(rec["bits"])[:n].reshape(rec["shape"])


def mine_false_positives(pred_dir, lits_root, classes=("Liver", "Tumor"), min_size=NEG_MIN_SIZE, device=None):
    """DataLoader/NF/input_pipeline_3d.py:187-219 `load_neg` for LiTS, on the device: for every
    predict-<PID>.nii.gz of pred_dir (what --save_predict writes) whose PID is in <lits_root>/meta.json, the 6-connected
    components of the predicted object class that hold >= min_size voxels and touch no labelled voxel of that class
    (ops.fp_mask3d) -> <lits_root>/neg3d/neg-<PID>.npz.  The object class is lits3d.label_map's fg_label: the tumour where it
    is a class, else the liver.  The prediction is read with the volume's mirror rule (as lits3d.prediction_box reads it), the
    labels come from the PNG store.  Returns [(pid, path, components, kept, voxels)]."""
    import torch

    from .. import ops
    from . import lits, lits3d
    _, fg_label = lits3d.label_map(classes)
    if int(min_size) < 1:
        raise ValueError("--min_size must be >= 1, got {}".format(min_size))
    device = device or torch.device("cuda", torch.cuda.current_device())
    root = Path(lits_root)
    with (root / "meta.json").open() as f:
        meta = {int(c["PID"]): c for c in json.load(f)}
    dst = root / NEG_DIR
    dst.mkdir(parents=True, exist_ok=True)
    files = []
    for p in Path(pred_dir).glob("predict-*.nii.gz"):
        stem = p.name[len("predict-"):-len(".nii.gz")]
        if stem.isdigit() and int(stem) in meta:
            files.append((int(stem), p))
    done = []
    for pid, path in sorted(files):
        _, pred = nii_kits.read_nii(path, out_dtype=np.uint8, special=28 <= pid < 48)
        want = tuple(int(v) for v in lits._maybe_json(meta[pid]["size"]))
        if tuple(pred.shape) != want:
            raise ValueError("{} holds a volume of shape {}, case {} has {}".format(path, tuple(pred.shape), pid, want))
        store = lits.SliceStore(root, [{"PID": pid, "size": list(want)}], device)
        out, counts, head = ops.fp_mask3d(torch.from_numpy(np.ascontiguousarray(pred)).to(device), store.lb, fg_label, fg_label,
                                          min_size=min_size, out_value=1, lab_scale=LB_SCALE)
        components, kept, voxels, _ = head.tolist()
        target = dst / "neg-{}.npz".format(pid)
        save_neg(target, out.cpu().numpy(), counts.cpu().numpy(), kept, components)
        del store, out
        done.append((pid, target, components, kept, voxels))
    return done


def main(argv=None):
    """python -m boxsegliver_amd.data.extract png <nii_dir> <lits_root>/png
       python -m boxsegliver_amd.data.extract neg3d <pred_dir> <lits_root> [--classes Liver Tumor] [--min_size 6]
       python -m boxsegliver_amd.data.extract hist <nii_dir> <lits_root>/feat [--mode train eval]
       python -m boxsegliver_amd.data.extract glcm <nii_dir> <lits_root>/feat --meta <lits_root>/meta.json [--mode train eval]
       python -m boxsegliver_amd.data.extract prior <lits_root>"""
    import argparse
    parser = argparse.ArgumentParser(prog="python -m boxsegliver_amd.data.extract", description=__doc__.split("\n")[0])
    sub = parser.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("png", help="NIfTI volumes -> PNG slices + meta.json")
    p.add_argument("nii_dir")
    p.add_argument("out_dir")
    p.add_argument("--only_meta", action="store_true")
    h = sub.add_parser("hist", help="NIfTI volumes -> per-slice histogram context features <out>/hist/<mode>/<PID>.npy")
    h.add_argument("nii_dir")
    h.add_argument("feat_dir")
    h.add_argument("--mode", nargs="+", choices=("train", "eval"), default=["train", "eval"])
    g = sub.add_parser("glcm", help="NIfTI volumes + meta.json -> per-slice co-occurrence texture context features "
                                    "<out>/glcm/<mode>/<PID>.npy")
    g.add_argument("nii_dir")
    g.add_argument("feat_dir")
    g.add_argument("--meta", required=True, help="the meta.json of the `png` sub-command")
    g.add_argument("--mode", nargs="+", choices=("train", "eval"), default=["train", "eval"])
    r = sub.add_parser("prior", help="<lits_root>/meta.json -> <lits_root>/prior.json, the simulated user prior of the "
                                     "propagated evaluation")
    r.add_argument("lits_root")
    n = sub.add_parser("neg3d", help="saved predictions predict-<PID>.nii.gz -> their false-positive objects "
                                     "<lits_root>/neg3d/neg-<PID>.npz, for liver_3d --hard_neg_from")
    n.add_argument("pred_dir")
    n.add_argument("lits_root")
    n.add_argument("--classes", nargs="+", default=["Liver", "Tumor"])
    n.add_argument("--min_size", type=int, default=NEG_MIN_SIZE, help="the smallest component that is kept, in voxels")
    a = parser.parse_args(argv)
    if a.cmd == "png":
        nii_3d_to_png(a.nii_dir, a.out_dir, a.only_meta)
    elif a.cmd == "neg3d":
        for pid, path, components, kept, voxels in mine_false_positives(a.pred_dir, a.lits_root, a.classes, a.min_size):
            print("case {}: {} components, {} kept, {} voxels -> {}".format(pid, components, kept, voxels, path))
    elif a.cmd == "prior":
        print(write_user_prior(a.lits_root))
    elif a.cmd == "glcm":
        for mode in a.mode:
            for path in dump_glcm_feature(a.nii_dir, a.feat_dir, mode, a.meta):
                print(path)
    else:
        for mode in a.mode:
            for path in dump_hist_feature(a.nii_dir, a.feat_dir, mode):
                print(path)


if __name__ == "__main__":
    main()
