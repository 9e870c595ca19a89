"""Spatial-guide propagation for the offline evaluation of a spatially guided GUNet -- the reference's
DataLoader/Liver/input_pipeline_g.py:1179-1513 (`EvalImage3DLoader`) as driven by evaluators/evaluator_liver.py:768-917
(`run_g`, `_predict_case_g`).

Each evaluated case is walked slice by slice, first upward ("Forward") and then downward ("Backward").  A simulated user
prior (<lits_root>/prior.json, `python -m boxsegliver_amd.data.extract prior <lits_root>`) places a Gaussian guide on the
middle slice of every tumour; after each slice the tumours the model predicted there become the guide of the next one.

Split of the work:
  * `Propagation` (host, small objects only): the guide objects of a slice (`start_slice`) and the reference's `last_pred`
    setter (`finish_slice`), which matches the predicted components to the guides and keeps the ones that propagate.
  * the per-slice component table and the guide image come from csrc (`ops.guide_components`, `ops.guide_render`) in the
    evaluator's device loop; `components_numpy` / `render_numpy` below restate both kernels in numpy for the host tests.
  * `EvalCases` serves the cases: `parse_case_eval(align=16, padding=25, padding_z=0)`, the slab loaders' resize, the
    context row of each slice.

The reference's behaviour is kept as it is, quirks included:
  1. z-range test with bound methods.  The reference tests `self.forward and ...` / `self.backward and ...` with the methods
     themselves, never called, so both conditions are always armed: in either sweep a matched tumour is dropped when
     `sid >= z[1] or sid <= z[0]`.
  2. `last_info` survives some resets.  A slice with no tumour predicted returns before `last_info.clear()`, so the previous
     slice's objects are propagated once more; and `last_info` is never reset between the two sweeps or between cases.
  3. Prior filtering and centre mapping.  A prior entry counts only if `min(stddev) > min_std` (strict); its centre is mapped
     into the network-size patch with Python `int()`, which truncates toward zero.
  4. Propagated objects.  centre = int32(median + box start) (truncation), stddev = max(f32(1.4826 MAD), min_std).
  5. Component rules.  4-connected components in raster order of their first pixel; one whose peak of mask x guide is below
     0.15 + 0.5 is ignored; otherwise it matches the guide whose centre equals its peak (the first maximum in raster order),
     else the first guide in np.argsort order of squared distance whose Wu line rises monotonically from the peak, else the
     reference's ValueError("Can not find corresponding guide!").
  6. Tumour mask.  The mask that feeds the next slice is argmax(mirror-averaged probabilities) == 2.
"""
import copy
import json
from collections import namedtuple
from pathlib import Path

import numpy as np
import scipy.ndimage as ndi

from ..utils import array_kits

SP_GUIDE_BG = 0.5
FILTER_THRESH = 0.15 + SP_GUIDE_BG          # input_pipeline_g.py: filter_thresh
PRIOR_COMMAND = "python -m boxsegliver_amd.data.extract prior <lits_root>"

# one predicted tumour component of a slice: peak = (y, x) of the first maximum of guide over it, center / stddev the raw
# float32 robust moments (no min_std floor), box = (y0, x0, y1, x1) inclusive
Component = namedtuple("Component", "root area box peak peak_value center stddev")


def load_prior(lits_root, real_sp=None):
    """The user prior: --real_sp <file> if given, else <lits_root>/prior.json."""
    path = Path(real_sp) if real_sp else Path(lits_root) / "prior.json"
    if not path.exists():
        raise FileNotFoundError("missing prior file {}; make it with `{}`".format(path, PRIOR_COMMAND))
    with path.open() as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ numpy restatements
def components_numpy(mask, guide):
    """unetk_guide_components restated: the components of a binary tumour mask [H, W] with their peaks on `guide`."""
    mask = np.asarray(mask) != 0
    guide = np.asarray(guide, np.float32)
    labeled, n = ndi.label(mask, ndi.generate_binary_structure(2, 1))
    out = []
    for i, sl in enumerate(ndi.find_objects(labeled)):
        obj = labeled[sl] == i + 1
        prod = obj * guide[sl]
        pk = np.unravel_index(prod.argmax(), prod.shape)
        points = np.transpose(np.nonzero(obj)).astype(np.float32)
        med = np.median(points, axis=0)
        std = np.float32(1.4826) * np.median(np.absolute(points - med), axis=0)
        first = np.flatnonzero(obj[0])[0] + sl[1].start
        out.append(Component(root=int(sl[0].start * mask.shape[1] + first), area=int(obj.sum()),
                             box=(sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1),
                             peak=(int(pk[0] + sl[0].start), int(pk[1] + sl[1].start)), peak_value=np.float32(prod.max()),
                             center=(med + np.array([sl[0].start, sl[1].start], np.float32)).astype(np.float32),
                             stddev=std.astype(np.float32)))
    return out


def render_numpy(objects, shape, discount):
    """unetk_guide_render restated: create_gaussian_distribution_v2(shape, centres, stddevs) * discount / 2 + 0.5 in
    float32, or 0.5 everywhere without objects.  objects: float32 [n, 4] = (cy, cx, sy, sx)."""
    objects = np.asarray(objects, np.float32).reshape(-1, 4)
    if len(objects) == 0:
        return np.full(shape, SP_GUIDE_BG, np.float32)
    coords = np.stack(np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij"), axis=-1).astype(np.float32)
    c = objects[:, None, None, :2]
    s = objects[:, None, None, 2:]
    d = np.exp(-np.sum((coords[None] - c) ** 2 / (2 * s * s), axis=-1)).max(axis=0)
    return d * discount / 2 + SP_GUIDE_BG


def parse_table(table, width, skip_low=False):
    """The host copy of an ops.guide_components table of an image `width` pixels wide -> ([Component], n_low); raises if
    the table overflowed.  skip_low: components whose peak is below FILTER_THRESH (they change nothing but the fact that
    the slice had a tumour) are only counted, in one vectorised test -- an early checkpoint can predict thousands."""
    t = np.asarray(table, np.int32)
    count, overflow = int(t[0]), int(t[1])
    if overflow:
        raise RuntimeError("{} tumour components on one slice exceed the table capacity {}".format(
            count, (len(t) - 4) // 12))
    rows = t[4:4 + 12 * count].reshape(count, 12)
    f = rows.view(np.float32)
    n_low = 0
    if skip_low:
        keep = f[:, 7] >= FILTER_THRESH
        n_low = int(count - keep.sum())
        rows, f = rows[keep], f[keep]
    return [Component(root=int(r[0]), area=int(r[1]), box=tuple(int(v) for v in r[2:6]),
                      peak=(int(r[6]) // width, int(r[6]) % width), peak_value=fr[7], center=fr[8:10].copy(),
                      stddev=fr[10:12].copy())
            for r, fr in zip(rows, f)], n_low


def ascent_line(img, x0, y0, x1, y1):
    """input_pipeline_g.py `ascent_line`: do the guide values along the Wu line from (x0, y0) to (x1, y1) never decrease?
    A forward line starts at its first pixel (read twice); a backward one starts at its last pixel and walks back to the
    first."""
    xs, ys, forward = array_kits.xiaolinwu_line(x0, y0, x1, y1)
    if forward:
        pre, path = img[ys[0], xs[0]], list(zip(xs, ys))
    else:
        pre, path = img[ys[-1], xs[-1]], list(zip(xs[:-1], ys[:-1]))[::-1]
    for x, y in path:
        cur = img[y, x]
        if not cur >= pre:
            return False
        pre = cur
    return True


# ------------------------------------------------------------------------------------------------ the state machine
class Propagation(object):
    """The guide bookkeeping of EvalImage3DLoader: `curr_info` (the guides of the current slice), `last_info` (the tumours
    propagated from the previous one).  One instance serves all cases of an evaluation (quirk 2)."""

    def __init__(self, user_info, min_std, discount, pshape):
        self.user_info = user_info
        self.min_std = float(min_std)
        self.discount = float(discount)
        self.pshape = tuple(int(v) for v in pshape[:2])
        self.last_info = []
        self.curr_info = []

    def start_slice(self, pid, sid, bbox, cshape):
        """process_slice's guide part: the prior entries of slice `sid` that pass the stddev filter, mapped into the
        patch, then the propagated objects.  Returns the objects as float32 [n, 4] = (cy, cx, sy, sx)."""
        self.curr_info = []
        slices = self.user_info[str(pid)]
        if str(sid) in slices:
            for x in copy.deepcopy(slices[str(sid)]):
                if np.min(x["stddev"]) > self.min_std:
                    x["center"][0] = int((x["center"][0] - bbox[1]) / cshape[1] * self.pshape[0])
                    x["center"][1] = int((x["center"][1] - bbox[0]) / cshape[2] * self.pshape[1])
                    self.curr_info.append(x)
        self.curr_info.extend(self.last_info)
        return self.objects()

    def objects(self):
        if not self.curr_info:
            return np.zeros((0, 4), np.float32)
        stddevs = [x["stddev"] for x in self.curr_info]
        assert np.min(stddevs) >= self.min_std, stddevs
        return np.concatenate([np.asarray([x["center"] for x in self.curr_info], np.float32),
                               np.asarray(stddevs, np.float32)], axis=1)

    def finish_slice(self, sid, components, guide, n_low=0):
        """The `last_pred` setter.  components: the slice's [Component] in root order; guide: the guide image the slice was
        given, or a callable returning it (read only when an ascent test is needed); n_low: components left out of the list
        because their peak is below the threshold.  Returns the decision of every listed component: "low" (below the
        threshold), "ended" (outside its guide's z-range) or the index of the kept object."""
        if not components and not n_low:
            return []                                  # quirk 2: last_info is kept
        self.last_info.clear()
        img = [None]

        def guide_image():
            if img[0] is None:
                img[0] = guide() if callable(guide) else guide
            return img[0]

        decisions = []
        for comp in components:
            if comp.peak_value < FILTER_THRESH:
                decisions.append("low")
                continue
            peak = np.asarray(comp.peak, dtype=np.int64)
            found = -1
            for j, obj in enumerate(self.curr_info):
                if np.all(peak == obj["center"]):
                    found = j
                    break
            if found < 0 and self.curr_info:
                distances = np.sum([(peak - obj["center"]) ** 2 for obj in self.curr_info], axis=1)
                for j in np.argsort(distances):
                    ctr = self.curr_info[j]["center"]
                    if ascent_line(guide_image(), peak[1], peak[0], ctr[1], ctr[0]):
                        found = j
                        break
            if found < 0:
                raise ValueError("Can not find corresponding guide!")
            z = self.curr_info[found]["z"]
            if sid >= z[1] or sid <= z[0]:             # quirk 1: both sweep conditions armed
                decisions.append("ended")
                continue
            std = np.maximum(np.asarray(comp.stddev, np.float32), [self.min_std] * 2)
            self.last_info.append({"z": copy.copy(z), "center": np.asarray(comp.center, np.float32).astype(np.int32).tolist(),
                                   "stddev": std.tolist()})
            decisions.append(len(self.last_info) - 1)
        return decisions


# ------------------------------------------------------------------------------------------------ the cases
class EvalCases(object):
    """prepare_next_case / gen_next_batch of EvalImage3DLoader without the model: per case the normalised volume resized
    to the network size (y, x, z with the context slices), its labels, its box, and the slice order of the two sweeps.
    This input side stays on the host (window and resize in numpy, one upload per case) whatever the evaluator's
    volumes_on says; only the zoom back of run_g follows that switch."""

    def __init__(self, data_list, config, proj_root=".", lits_root=None, context=None):
        self.data_list = list(data_list)[int(getattr(config, "eval_skip_num", 0)):]
        n = int(getattr(config, "eval_num", -1))
        self.num_cases = n if n > 0 else len(self.data_list)
        self.config, self.proj_root, self.context = config, proj_root, context
        self.pshape = (int(config.im_height), int(config.im_width), int(config.im_channel))

    def __iter__(self):
        from . import lits
        for case in self.data_list[:self.num_cases]:
            pid, vol_path, _, bbox, _, cshape, lhc, rhc, volume, segmentation = lits.parse_case_eval(
                case, 16, 25, 0, self.pshape[2], parse_label=True, proj_root=self.proj_root)
            volume = lits.cv2_resize_linear(volume, self.pshape[:2])
            rows = self.context.case(case, 0) if self.context is not None else None
            yield {"case": case, "pid": pid, "vol_path": vol_path, "bbox": bbox, "cshape": cshape, "lhc": lhc, "rhc": rhc,
                   "volume": volume, "segmentation": segmentation, "context": rows}


def sweeps(cshape, lhc, rhc):
    """gen_next_batch's slice order: [(direction, idx)], idx the centre index into the (context-padded) z axis."""
    up = [("Forward", idx) for idx in range(lhc, cshape[0] - rhc)]
    down = [("Backward", idx) for idx in range(cshape[0] - rhc - 1, lhc - 1, -1)]
    return up + down
