"""Guide-propagation fixtures pinned on the REFERENCE ITSELF (build container only): the state machine of the reference's
DataLoader/Liver/input_pipeline_g.py `EvalImage3DLoader` (process_slice + the `last_pred` setter) driven with scripted
tumour masks, and DataLoader/Liver/extract.py `simulate_user_prior` on tests/golden/ref_meta_excerpt.json, written to
tests/golden/ref_propagation.npz.

    python tests/golden/make_propagation_fixtures.py     # needs the reference checkout; rewrites ref_propagation.npz

The modules import tensorflow, cv2, skimage, medpy, nibabel and SimpleITK at module level for functions the state machine
does not use; stand-ins are put into sys.modules first.  The loader gets its prior through `real_sp` (a temporary file) and
its case fields are set directly (no prepare_next_case, no volumes).  `simulate_user_prior` reads and writes its own
`prepare/` directory next to extract.py: the module's __file__ is pointed into a temporary directory for the call.

Scenario (48 x 48 patches, two cases, one loader): a slice without guides, blobs below the threshold, two blobs touching only
at a corner, centre hits, an ascent-line match, tumours dropped at both ends of their z-range, empty slices (objects carry
over), carry-over between the sweeps and between the cases, and a slice that ends in "Can not find corresponding guide!".
tests/test_propagation_host.py replays it on boxsegliver_amd.data.propagate."""
import argparse
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
PSHAPE = (48, 48, 3)
MIN_STD = 2.0
DISCOUNT = 0.85


class _Anything(types.ModuleType):
    """A stand-in module: every attribute is another stand-in, callable, usable as a decorator or a base class."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = _Anything(self.__name__ + "." + name)
        setattr(self, name, sub)
        return sub

    def __call__(self, *a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return _Anything(self.__name__ + "()")

    def __mro_entries__(self, bases):
        return (object,)


STUBBED = ("tensorflow", "tensorflow_estimator", "cv2", "tqdm", "SimpleITK", "nibabel", "skimage", "medpy")


class _StubFinder(object):
    """Serves a stand-in for every module under STUBBED, submodules included."""

    def find_spec(self, name, path=None, target=None):
        import importlib.machinery
        if name.split(".")[0] in STUBBED:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _Anything(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def _import_reference():
    sys.meta_path.insert(0, _StubFinder())
    import tensorflow.python.platform.tf_logging  # noqa: F401
    logging = sys.modules["tensorflow.python.platform.tf_logging"]
    logging.info = logging.warning = lambda *a, **k: None
    sys.path.insert(0, REF)
    from DataLoader.Liver import extract, input_pipeline_g
    return extract, input_pipeline_g


def _decoded(case):
    return {k: (json.loads(v) if isinstance(v, str) and k != "vol_case" and k != "lab_case" else v) for k, v in case.items()}


def prior_of_excerpt(extract):
    excerpt = json.load(open(os.path.join(HERE, "ref_meta_excerpt.json")))["cases"]
    meta = [_decoded(c) for c in excerpt]
    saved = extract.__file__
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "prepare"))
        with open(os.path.join(tmp, "prepare", "meta.json"), "w") as f:
            json.dump(meta, f)
        extract.__file__ = os.path.join(tmp, "extract.py")
        try:
            extract.simulate_user_prior("prior.json")
        finally:
            extract.__file__ = saved
        with open(os.path.join(tmp, "prepare", "prior.json")) as f:
            return f.read()


# prior in ORIGINAL image coordinates; case 7's box starts at (y 20, x 10), case 8's at (0, 0); both map 96 -> 48
PRIOR = {
    "7": {"104": [{"z": [101, 108], "center": [60.0, 51.0], "stddev": [3.0, 4.0]},          # -> (20, 20): int(20.5) = 20
                  {"z": [104, 106], "center": [100.0, 90.0], "stddev": [2.5, 2.5]},          # -> (40, 40), ends at once
                  {"z": [103, 106], "center": [15.0, 30.0], "stddev": [2.2, 3.0]},           # -> int(-2.5) = -2: truncation
                  {"z": [101, 108], "center": [70.0, 70.0], "stddev": [2.0, 5.0]},           # min == min_std: filtered
                  {"z": [101, 108], "center": [70.0, 70.0], "stddev": [2.5, 1.5]}],          # filtered
          "105": [{"z": [100, 111], "center": [80.0, 30.0], "stddev": [3.5, 3.0]}]},         # -> (30, 10)
    "8": {"51": [{"z": [51, 53], "center": [48.0, 48.0], "stddev": [5.0, 5.0]},
                 {"z": [50, 54], "center": [-4.0, 48.0], "stddev": [6.0, 6.0]}]},          # -> (-2, 24): rows wrap
}
CASES = [
    {"pid": 7, "bbox": [10, 20, 100, 105, 115, 110], "cshape": [13, 96, 96]},
    {"pid": 8, "bbox": [0, 0, 50, 95, 95, 53], "cshape": [6, 96, 96]},
]


def _blob(mask, cy, cx, r=1):
    mask[max(cy - r, 0):cy + r + 1, max(cx - r, 0):cx + r + 1] = 1


def script(pid, direction, sid, curr, guide, ascent_line):
    """The tumour mask the 'model' predicts on a slice, given the guides of the slice."""
    m = np.zeros(PSHAPE[:2], np.uint8)
    centres = [tuple(int(v) for v in o["center"]) for o in curr]
    if pid == 7 and direction == "Forward" and sid == 100:
        _blob(m, 5, 5)                                        # no guide at all: below the threshold
    elif pid == 7 and direction == "Forward" and sid == 102:
        _blob(m, 10, 10)                                      # two blobs touching at a corner, both below the threshold
        _blob(m, 13, 13)
    elif pid == 7 and direction == "Forward" and sid == 104:
        m[23:26, 22:25] = 1                                   # next to (20, 20), not on it: ascent-line match
        _blob(m, 40, 40, 2)                                   # centre hit on a tumour whose z-range starts here: ended
        _blob(m, 5, 44)                                       # far from every guide: below the threshold
    elif pid == 7 and direction == "Forward" and sid == 105:
        for cy, cx in centres:
            _blob(m, cy, cx)
        cy, cx = centres[0]                                   # the prior (30, 10): a corner neighbour that ascends to it
        _blob(m, cy + 3, cx + 3)
    elif pid == 7 and sid in (106,) or (pid == 7 and direction == "Backward" and sid == 100):
        pass                                                  # empty: objects carry over
    elif pid == 8 and sid == 51:
        # a single pixel whose every Wu line to a guide centre dips somewhere -- here the line to the centre above the
        # patch reads the guide's last rows through numpy's negative indices: the reference's ValueError
        cand = [(y, x) for y in range(PSHAPE[0]) for x in range(PSHAPE[1])
                if guide[y, x] >= 0.65 and (y, x) not in centres
                and not any(ascent_line(guide, x, y, cx, cy) for cy, cx in centres)]
        assert cand, "no failing pixel"
        m[cand[0]] = 1
    else:
        for cy, cx in centres:
            if 0 <= cy < PSHAPE[0] and 0 <= cx < PSHAPE[1]:
                _blob(m, cy, cx)
    return m


def run_scenario(ipg, prior_file):
    cfg = argparse.Namespace(eval_skip_num=0, eval_num=-1, mode="eval", min_std=MIN_STD, im_height=PSHAPE[0],
                             im_width=PSHAPE[1], im_channel=PSHAPE[2], real_sp=prior_file, eval_mirror=False, random_flip=0,
                             eval_discount=DISCOUNT, save_sp_guide=False)
    loader = ipg.EvalImage3DLoader([None], context_guide=False, spatial_guide=True, config=cfg)
    steps = []
    for case in CASES:
        loader.pid, loader.spid, loader.bbox, loader.cshape = case["pid"], str(case["pid"]), case["bbox"], case["cshape"]
        loader.lhc = loader.rhc = 1
        loader.volume = np.zeros((1,) + PSHAPE[:2] + (case["cshape"][0],), np.float32)
        order = [("Forward", i) for i in range(1, case["cshape"][0] - 1)] + \
            [("Backward", i) for i in range(case["cshape"][0] - 2, 0, -1)]
        for direction, idx in order:
            loader.direction = direction
            batch = next(loader.process_slice({"images": None, "context": None, "sp_guide": None, "mirror": 0}, idx))
            guide = batch["sp_guide"][0, :, :, 0].copy()
            curr = copy.deepcopy(loader.curr_info)
            mask = script(case["pid"], direction, loader.sid, curr, guide, ipg.EvalImage3DLoader.ascent_line)
            error = ""
            try:
                loader.last_pred = mask[None, :, :, None]
            except ValueError as e:
                error = str(e)
            steps.append({"pid": case["pid"], "sid": loader.sid, "direction": direction, "mask": mask, "guide": guide,
                          "curr": curr, "last": copy.deepcopy(loader.last_info), "error": error})
            if error:
                return steps
    return steps


def main():
    extract, ipg = _import_reference()
    out = {"prior_json": np.array(prior_of_excerpt(extract))}
    with tempfile.TemporaryDirectory() as tmp:
        prior_file = os.path.join(tmp, "prior.json")
        with open(prior_file, "w") as f:
            json.dump(PRIOR, f)
        steps = run_scenario(ipg, prior_file)
    out["scenario_prior"] = np.array(json.dumps(PRIOR))
    out["cases"] = np.array(json.dumps(CASES))
    out["masks"] = np.stack([s["mask"] for s in steps])
    keep = [i for i, s in enumerate(steps) if s["pid"] == 8 or s["sid"] in (100, 104, 105)]
    out["guide_steps"] = np.array(keep, np.int32)
    out["guides"] = np.stack([steps[i]["guide"] for i in keep]).astype(np.float32)
    out["steps"] = np.array(json.dumps([{k: s[k] for k in ("pid", "sid", "direction", "curr", "last", "error")}
                                        for s in steps]))
    np.savez_compressed(os.path.join(HERE, "ref_propagation.npz"), **out)
    for s in steps:
        print(s["pid"], s["direction"], s["sid"], "curr", [o["center"] for o in s["curr"]], "last",
              [o["center"] for o in s["last"]], s["error"])
    print("wrote", os.path.join(HERE, "ref_propagation.npz"), os.path.getsize(os.path.join(HERE, "ref_propagation.npz")))


if __name__ == "__main__":
    main()
