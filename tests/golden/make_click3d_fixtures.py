"""3-D click fixtures pinned on the REFERENCE ITSELF (build container only): DataLoader/misc.py `volume_crop` and
DataLoader/NF/input_pipeline_3d.py `gen_kernel` / `inter_simulation` run on the label volumes of tests/click3d_shapes.py,
written to tests/golden/ref_clicks3d.json (integers only).

    python tests/golden/make_click3d_fixtures.py     # needs the reference checkout; rewrites ref_clicks3d.json

The module imports tensorflow, GeodisTK, skimage, cv2, nibabel and others at module level for functions the click simulator
does not use; the stand-ins of make_propagation_fixtures.py are put into sys.modules first.  The reference spells the erosion
element's dtype `np.bool`, an alias that numpy 2 no longer has: it is set before the import.

A record is made the way the reference makes a sample: volume_crop(label volume, centre, (D, ch, cw)) gives the label patch
and its slices (recorded: the crop clamp is pinned too), gen_kernel(nf=True, image patch, label patch, cfg) returns the
clicks.  A case shallower than D is the project's documented deviation (tests/lits3d_ref.py: cropped from slice 0, padded with
label-0 slices -- volume_crop would index with a negative start): its patch is built that way here and the record says so
("box_via": "padded").  numpy's generator is scripted from the record's click_tab row as make_click_fixtures.py scripts it:
randint returns n_fg for the foreground call (low == 1) and n_bg for the background call (low == 0), sample returns 0.75 for
strategy 1 and 0.25 for strategy 3, and the k-th choice(count) of a call returns (draw[k] * count) >> 32.  Every
(rank, count) the reference asked for is recorded next to the clicks.

gen_kernel fixes margin 3, step 10, band 40, N 5.  Records with other parameters call inter_simulation directly, foreground
with strategy 0 and background with the row's strategy, scripted the same way.

Where the reference raises, the record says so: an all-object patch has an empty background mask, the reference converts the
mean of no voxel to int32 and fails (with this numpy: an index of -2^31).  That record carries the project's documented deviation (no background click) and the
foreground clicks of a direct inter_simulation call."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import click3d_shapes as c3  # noqa: E402
import make_click_fixtures as mcf  # noqa: E402
import make_propagation_fixtures as mpf  # noqa: E402


def _import_reference():
    if not hasattr(np, "bool"):
        np.bool = bool                                                            # input_pipeline_3d.py:290
    mpf.STUBBED = tuple(mpf.STUBBED) + ("GeodisTK", "skimage", "cv2", "nibabel")
    sys.meta_path.insert(0, mpf._StubFinder())
    import tensorflow.python.platform.tf_logging  # noqa: F401
    logging = sys.modules["tensorflow.python.platform.tf_logging"]
    logging.info = logging.warning = lambda *a, **k: None
    sys.path.insert(0, mpf.REF)
    from DataLoader import misc
    from DataLoader.NF import input_pipeline_3d as pipe
    return misc, pipe


class Config(object):
    fp_sample = False
    use_cascade = False


def _pts(a):
    a = np.asarray(a)
    assert a.ndim == 2 and a.shape[1] == 3 and np.all(a == np.floor(a))
    return [[int(z), int(y), int(x)] for z, y, x in a]


def record(misc, pipe, rid, vname, centre, depth_out, crop, params, row):
    volume = c3.build(vname)
    shape = (int(depth_out), int(crop[0]), int(crop[1]))
    if volume.shape[0] >= depth_out:
        patch, slices = misc.volume_crop(volume, tuple(centre), shape)
        box = [int(s.start) for s in slices] + [int(s.stop) for s in slices]
        via = "volume_crop"
    else:                                                                         # the deviation: from slice 0, padded
        _, (sy, sx) = misc.img_crop(volume, 0, 1, tuple(centre[1:]), tuple(crop))
        patch = np.zeros(shape, volume.dtype)
        patch[:volume.shape[0]] = volume[:, sy, sx]
        box = [0, int(sy.start), int(sx.start), shape[0], int(sy.stop), int(sx.stop)]
        via = "padded"
    assert patch.shape == shape
    lab_patch = np.clip(patch, 0, 1).astype(np.int8)
    img_patch = np.zeros(lab_patch.shape + (1,), np.float32)
    rec = {"id": rid, "volume": vname, "centre": list(centre), "depth": int(depth_out), "crop": list(crop), "params": list(params),
           "row": [int(v) for v in row], "box": box, "box_via": via, "raises": ""}
    margin, step, band, n_max = params
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                           # the mean of an empty patch
        if tuple(params) == c3.REF_CLICKS:
            rec["via"] = "gen_kernel"
            out = None
            with mcf.Script(row) as script:
                try:
                    out = pipe.gen_kernel(True, img_patch, lab_patch.copy(), Config())
                except (ValueError, IndexError) as e:                            # NaN -> int32: an error or a wild index
                    rec["raises"] = type(e).__name__ + ": " + str(e)
            if rec["raises"]:
                assert not (1 - lab_patch).any(), "only an all-object patch may fail"
                with mcf.Script(row) as script:
                    fg = pipe.inter_simulation(lab_patch.copy(), margin=margin, step=step, N=n_max, bg=False, strategy=0)
                bg = np.zeros((0, 3))
                script.asked["bg"] = []
            else:
                _, lab_out, fg, bg = out
                assert np.array_equal(lab_out, lab_patch)
        else:
            rec["via"] = "inter_simulation"
            with mcf.Script(row) as script:
                fg = pipe.inter_simulation(lab_patch.copy(), margin=margin, step=step, N=n_max, bg=False, strategy=0) \
                    if lab_patch.max() > 0 else np.zeros((0, 3))
                bg = pipe.inter_simulation(1 - lab_patch, margin=margin, step=step, N=n_max, bg=True, d=band,
                                           strategy=int(row[2]))
    rec["fg"], rec["bg"] = _pts(fg), _pts(bg)
    rec["asked"] = script.asked
    return rec


def main():
    misc, pipe = _import_reference()
    volumes = {}
    for name, (shape, slices) in c3.VOLUMES.items():
        count, index_sum = c3.checksum(c3.build(name))
        volumes[name] = {"shape": [len(slices)] + list(shape), "popcount": count, "index_sum": index_sum}
    records = []
    for rid, vname, centre, depth_out, crop, params, rows in c3.RECORDS:
        for row in rows:
            records.append(record(misc, pipe, rid, vname, centre, depth_out, crop, params, row))
            r = records[-1]
            print(rid, r["row"][:3], r["box"], "fg", r["fg"], "bg", r["bg"], r["raises"])
    path = os.path.join(HERE, "ref_clicks3d.json")
    with open(path, "w") as f:
        f.write("{\n\"volumes\": " + json.dumps(volumes, sort_keys=True) + ",\n\"records\": [\n")
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in records))
        f.write("\n]\n}\n")
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
