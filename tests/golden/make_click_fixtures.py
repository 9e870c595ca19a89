"""Click fixtures pinned on the REFERENCE ITSELF (build container only): DataLoader/misc.py `img_crop` and
DataLoader/NF/input_pipeline_g_simply.py `gen_kernel` / `inter_simulation` run on the label slices of tests/click_shapes.py,
written to tests/golden/ref_clicks.json (integers only).

    python tests/golden/make_click_fixtures.py     # needs the reference checkout; rewrites ref_clicks.json

The module imports tensorflow, GeodisTK and others at module level for functions the click simulator does not use; the
stand-ins of make_propagation_fixtures.py are put into sys.modules first.  A record is made the way the reference makes a
sample: img_crop(label volume, pz, 1, centre, crop) gives the label patch and its slices (recorded: the crop clamp is pinned
too), gen_kernel(nf=True, queue, image patch, label patch, fp_sample=False) puts the clicks into a list-backed queue.  numpy's
generator is scripted from the record's click_tab row (data/lits_inter.draw_click_tab has the columns): randint returns n_fg
for the foreground call (low == 1) and n_bg for the background call (low == 0), sample returns 0.75 for strategy 1 and 0.25
for strategy 3, and the k-th choice(count) of a call returns (draw[k] * count) >> 32.  Every (rank, count) the reference asked
for is recorded next to the clicks.

gen_kernel fixes margin 3, step 10, band 40, N 5.  Records with other parameters (SMALL_CLICKS, CAP255_CLICKS) call
inter_simulation directly, foreground with strategy 0 and background with the row's strategy, scripted the same way.

Where the reference raises, the record says so: an all-object crop has an empty background mask, the reference converts the
mean of no pixel to int and fails.  That record carries the project's documented deviation (no background click) and the
foreground clicks of a direct inter_simulation call."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import click_shapes as cs  # noqa: E402
import make_propagation_fixtures as mpf  # noqa: E402


def _import_reference():
    mpf.STUBBED = tuple(mpf.STUBBED) + ("GeodisTK",)
    sys.meta_path.insert(0, mpf._StubFinder())
    import tensorflow.python.platform.tf_logging  # noqa: F401
    logging = sys.modules["tensorflow.python.platform.tf_logging"]
    logging.info = logging.warning = lambda *a, **k: None
    sys.path.insert(0, mpf.REF)
    from DataLoader import misc
    from DataLoader.NF import input_pipeline_g_simply as pipe
    return misc, pipe


class Script(object):
    """np.random.randint / sample / choice answering from one click_tab row; `asked` collects (kind, rank, count)."""

    def __init__(self, row):
        self.row = [int(v) for v in row]
        self.kind = None
        self.k = 0
        self.asked = {"fg": [], "bg": []}

    def randint(self, low, high=None):
        self.kind, self.k = ("fg", 0) if low == 1 else ("bg", 0)
        n = self.row[0] if low == 1 else self.row[1]
        assert low <= n < high, (low, n, high)
        return n

    def sample(self):
        return {1: 0.75, 3: 0.25}[self.row[2]]

    def choice(self, count):
        base = 4 if self.kind == "fg" else 8
        rank = (self.row[base + self.k] * int(count)) >> 32
        self.asked[self.kind].append([int(rank), int(count)])
        self.k += 1
        return rank

    def __enter__(self):
        self.saved = np.random.randint, np.random.sample, np.random.choice
        np.random.randint, np.random.sample, np.random.choice = self.randint, self.sample, self.choice
        return self

    def __exit__(self, *exc):
        np.random.randint, np.random.sample, np.random.choice = self.saved


class ListQueue(list):
    def put(self, item):
        self.append(item)


def _pts(a):
    a = np.asarray(a)
    assert a.ndim == 2 and a.shape[1] == 2 and np.all(a == np.floor(a))
    return [[int(y), int(x)] for y, x in a]


def record(misc, pipe, sid, mask_name, centre, crop, params, row):
    shape, ellipses, rects = cs.MASKS[mask_name]
    volume = cs.build(shape, ellipses, rects)[None]                           # one slice: pz = 0, channel = 1
    patch, slices = misc.img_crop(volume, 0, 1, tuple(centre), tuple(crop))
    lab_patch = np.clip(patch[0], 0, 1).astype(np.int8)
    img_patch = np.zeros(lab_patch.shape + (1,), np.float32)
    rec = {"id": sid, "mask": mask_name, "centre": list(centre), "crop": list(crop), "params": list(params),
           "row": [int(v) for v in row], "slices": [int(slices[0].start), int(slices[0].stop), int(slices[1].start),
                                                    int(slices[1].stop)], "raises": ""}
    margin, step, band, n_max = params
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # the mean of an empty slice
        if tuple(params) == cs.REF_CLICKS:
            rec["via"] = "gen_kernel"
            queue = ListQueue()
            with Script(row) as script:
                try:
                    pipe.gen_kernel(True, queue, img_patch, lab_patch.copy(), False)
                except ValueError as e:
                    rec["raises"] = "ValueError: " + str(e)
            if rec["raises"]:
                assert not (1 - lab_patch).any(), "only an all-object crop may fail"
                with Script(row) as script:
                    fg = pipe.inter_simulation(lab_patch.copy(), margin=margin, step=step, N=n_max, bg=False, strategy=0)
                bg = np.zeros((0, 2))
                script.asked["bg"] = []
            else:
                (_, lab_out, fg, bg), = queue
                assert np.array_equal(lab_out, lab_patch)
        else:
            rec["via"] = "inter_simulation"
            with Script(row) as script:
                fg = pipe.inter_simulation(lab_patch.copy(), margin=margin, step=step, N=n_max, bg=False, strategy=0) \
                    if lab_patch.max() > 0 else np.zeros((0, 2))
                bg = pipe.inter_simulation(1 - lab_patch, margin=margin, step=step, N=n_max, bg=True, d=band,
                                           strategy=int(row[2]))
    rec["fg"], rec["bg"] = _pts(fg), _pts(bg)
    rec["asked"] = script.asked
    return rec


def main():
    misc, pipe = _import_reference()
    masks = {}
    for name, (shape, ellipses, rects) in cs.MASKS.items():
        count, index_sum = cs.checksum(cs.build(shape, ellipses, rects))
        masks[name] = {"shape": list(shape), "popcount": count, "index_sum": index_sum}
    records = []
    for sid, mask_name, centre, crop, params, rows in cs.SHAPES:
        for row in rows:
            records.append(record(misc, pipe, sid, mask_name, centre, crop, params, row))
            r = records[-1]
            print(sid, r["row"][:3], r["slices"], "fg", r["fg"], "bg", r["bg"], r["raises"])
    path = os.path.join(HERE, "ref_clicks.json")
    with open(path, "w") as f:
        f.write("{\n\"masks\": " + json.dumps(masks, sort_keys=True) + ",\n\"records\": [\n")
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in records))
        f.write("\n]\n}\n")
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
