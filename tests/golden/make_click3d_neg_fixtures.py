"""Hard-negative click fixtures pinned on the REFERENCE ITSELF (build container only): DataLoader/NF/input_pipeline_3d.py
`gen_kernel` with cfg.fp_sample = True -- i.e. on lab_patch + 10 * neg_patch -- and `inter_simulation(strategy=4, neg_patch=...)`
run on the label volumes of tests/click3d_shapes.py and the false-positive masks of tests/hard_neg_ref.py, written to
tests/golden/ref_clicks3d_neg.json (integers only).

    python tests/golden/make_click3d_neg_fixtures.py     # needs the reference checkout; rewrites ref_clicks3d_neg.json

The reference is imported and numpy's generator scripted from the record's click_tab row exactly as make_click3d_fixtures.py
does it (its helpers are imported): every (rank, count) the reference asked for is recorded next to the clicks.  With false
positives in the patch gen_kernel takes strategy 4 without drawing the strategy coin.  The label patch and the false-positive
patch are cut by the reference's volume_crop with the same slices; a case shallower than D is padded with empty slices, the
project's documented deviation.

gen_kernel fixes margin 3, step 10, band 40, N 5; records with other parameters call inter_simulation directly: the foreground
with strategy 0, the background with strategy 4 and the false-positive patch -- or, without a false positive in the patch, with
the row's strategy, as gen_kernel would choose."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))         # hard_neg_ref's helpers import the package
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import click3d_shapes as c3  # noqa: E402
import hard_neg_ref as hn  # noqa: E402
import make_click3d_fixtures as m3  # noqa: E402
import make_click_fixtures as mcf  # noqa: E402


class Config(object):
    fp_sample = True
    use_cascade = False


def _cut(misc, volume, centre, shape):
    """(patch, box, via) of one volume, as make_click3d_fixtures.record cuts the label patch."""
    if volume.shape[0] >= shape[0]:
        patch, slices = misc.volume_crop(volume, tuple(centre), shape)
        return patch, [int(s.start) for s in slices] + [int(s.stop) for s in slices], "volume_crop"
    _, (sy, sx) = misc.img_crop(volume, 0, 1, tuple(centre[1:]), tuple(shape[1:]))
    patch = np.zeros(shape, volume.dtype)
    patch[:volume.shape[0]] = volume[:, sy, sx]
    return patch, [0, int(sy.start), int(sx.start), shape[0], int(sy.stop), int(sx.stop)], "padded"


def record(misc, pipe, rid, nname, centre, depth_out, crop, params, row, same_as):
    vname = hn.NEG_MASKS[nname][0]
    volume, neg = c3.build(vname), hn.build_neg(nname)
    shape = (int(depth_out), int(crop[0]), int(crop[1]))
    patch, box, via = _cut(misc, volume, centre, shape)
    neg_patch, neg_box, _ = _cut(misc, neg, centre, shape)
    assert box == neg_box and patch.shape == neg_patch.shape == shape
    lab_patch = np.clip(patch, 0, 1).astype(np.int8)
    neg_patch = np.clip(neg_patch, 0, 1).astype(np.int8)
    img_patch = np.zeros(shape + (1,), np.float32)
    rec = {"id": rid, "neg": nname, "volume": vname, "centre": list(centre), "depth": int(depth_out), "crop": list(crop),
           "params": list(params), "row": [int(v) for v in row], "box": box, "box_via": via, "same_as": same_as or "",
           "neg_in_patch": int(neg_patch.sum())}
    margin, step, band, n_max = params
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with mcf.Script(row) as script:
            if tuple(params) == c3.REF_CLICKS:
                rec["via"] = "gen_kernel"
                _, lab_out, fg, bg = pipe.gen_kernel(True, img_patch, lab_patch + 10 * neg_patch, Config())
                assert np.array_equal(lab_out, lab_patch)
            else:
                rec["via"] = "inter_simulation"
                fg = pipe.inter_simulation(lab_patch.copy(), margin=margin, step=step, N=n_max, bg=False, strategy=0) \
                    if lab_patch.max() > 0 else np.zeros((0, 3))
                if neg_patch.max() > 0:
                    bg = pipe.inter_simulation(1 - lab_patch, margin=margin, step=step, N=n_max, bg=True, d=band, strategy=4,
                                               neg_patch=neg_patch)
                else:
                    bg = pipe.inter_simulation(1 - lab_patch, margin=margin, step=step, N=n_max, bg=True, d=band,
                                               strategy=int(row[2]))
    rec["fg"], rec["bg"] = m3._pts(fg), m3._pts(bg)
    rec["asked"] = script.asked
    return rec


def main():
    misc, pipe = m3._import_reference()
    masks = {}
    for name in hn.NEG_MASKS:
        count, index_sum = c3.checksum(hn.build_neg(name))
        masks[name] = {"volume": hn.NEG_MASKS[name][0], "popcount": count, "index_sum": index_sum}
    records = []
    for rid, nname, centre, depth_out, crop, params, rows, same_as in hn.RECORDS:
        for row in rows:
            records.append(record(misc, pipe, rid, nname, centre, depth_out, crop, params, row, same_as))
            r = records[-1]
            print(rid, r["row"][:3], r["box"], r["neg_in_patch"], "fg", r["fg"], "bg", r["bg"])
    path = os.path.join(HERE, "ref_clicks3d_neg.json")
    with open(path, "w") as f:
        f.write("{\n\"masks\": " + json.dumps(masks, sort_keys=True) + ",\n\"records\": [\n")
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in records))
        f.write("\n]\n}\n")
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
