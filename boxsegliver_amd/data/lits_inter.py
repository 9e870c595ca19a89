"""LiTS training input pipeline for the click-guided nets (UNetInter, SmallUNet, InterUNet, LGNet): 2-D samples cropped,
z-scored, resized, flipped and augmented on the device from the resident slice store, with the user clicks SIMULATED on
the device and rendered into `sp_guide`.  Sub-command `liver_inter` of both entry points.

The reference feeds these nets from its NF data (`nf_inter`, DataLoader/NF/input_pipeline_g_simply.py); it has no LiTS
pipeline for them.  The semantics here are that pipeline's, the volumes are the LiTS cases of `data/lits.SliceStore`:
  * :564-636 `gen_batch` -> `lits3d.PatchSampler` with shape (im_channel, H, W): which cases, which centres, zoom, and the
    draws the reference leaves to TensorFlow (flip coins, gamma);
  * :435-527 `data_processing`, DataLoader/misc.py:108-129 `img_crop` -> `unetk_lits_inter_batch` (csrc/lits_inter.hip);
  * :346-412 `inter_simulation` as :530-561 `gen_kernel` calls it (a pool of host processes in the reference) ->
    `unetk_lits_clicks`, from per-sample draws made here (`draw_click_tab`);
  * utils/image_ops.py:396-434 `create_spatial_guide_2d` + the resize -> `unetk_click_guide`;
  * :471-496 the geodesic guide -> `--geodesic_guide`: `unetk_lits_inter_center` (the half-resolution centre channel) and
    `unetk_click_geodesic` (csrc/lits_geodesic.hip), one workgroup per (sample, kind) relaxing to convergence in one launch.
    The reference grows it with GeodisTK on the host; here the distance is builder-defined (include/unetk.h, DESIGN.md 7.3.7.1:
    the float32 shortest path on the 8-connected grid, restated in tests/lits_geodesic_ref.py), so it has a flag of its own
    and `--geodesic`, which promises GeodisTK's numbers, stays refused.  It needs --use_spatial; --local_enhance and --stddev
    are ignored under it, as the reference ignores them under --geodesic (:447, :471).
TensorFlow does not run here: the arithmetic is pinned by the restatement in tests/lits_inter_ref.py, which cites the same
lines and uses scipy's `binary_erosion` literally ("parity unpinned").

A batch costs the host one sampler draw and ONE pinned upload (the int32 sample table and the click draws); nothing on the
batch path reads from the device.  The kernels' status word is read where an evaluation synchronises anyway.

The nets are binary, as on NF: `--classes Liver` makes the object stored label >= 1 (tumour counting as liver),
`--classes Tumor` stored label >= 2; labels are {0, 1} and the sampler's forced class is the object.

Not built: --geodesic (GeodisTK's own numbers; see --geodesic_guide), --fp_sample / --sample_neg (false-positive caches of earlier runs), --downsampling,
--use_context, and --mode eval / infer of this sub-command (evaluators/evaluator_nf.py).  The click-guided nets are scored
offline by entry/main_eval.py, the reference's own script for it.
Deviations: a crop that is all object gives no background click (the reference fails converting NaN), and a crop without a
non-zero voxel is all zeros (TensorFlow's moments of an empty tensor are NaN)."""
import numpy as np
import torch

from .. import _abi, ops
from ..utils import distribution_utils
from . import flagsets, lits, lits3d

CLICKS = (3, 10, 40, 5)            # gen_kernel :548-560: margin, step, N; d = 40 for the background band
OBJECT_LABEL = {("Liver",): 1, ("Tumor",): 2}
MAX_CHANNELS = 7
STATUS_BITS = ((1, "a forced sample's rank was beyond the object count of its slice (the per-slice counts do not match the store)"),
               (2, "a sample's centre slice lay outside its case"),
               (4, "a row of click draws was out of range"),
               (8, "a geodesic guide reached its sweep bound before it converged"))


def add_arguments(parser):
    """The flag group of `nf_inter` (input_pipeline_g_simply.py:50-109; names / defaults verbatim, data/flagsets.py) +
    --lits_root and --seed as the other LiTS sub-commands add them."""
    flagsets.add_arguments(parser, "liver_inter")
    parser.add_argument("--lits_root", type=str, default="data/LiTS", help="where png/, meta.json and k_folds.txt live")
    parser.add_argument("--seed", type=int, default=1234)
    parser.add_argument("--geodesic_guide", action="store_true",
                        help="With --use_spatial: the guide is the geodesic distance from the clicks through the half-resolution "
                             "centre channel (this project's float32 shortest-path definition, not GeodisTK's)")


def object_label(classes):
    """--classes -> the stored label from which a voxel is the object: `Liver` 1 (tumour counts as liver), `Tumor` 2."""
    classes = tuple(classes)
    if classes not in OBJECT_LABEL:
        raise ValueError("`liver_inter` trains binary nets: --classes Liver or --classes Tumor, got {}".format(" ".join(classes)))
    return OBJECT_LABEL[classes]


def refuse_unbuilt_flags(args):
    """Refuses the flags of the `liver_inter` group that are not built, naming the flag (training and entry.main_eval)."""
    if getattr(args, "geodesic", False):
        raise NotImplementedError("--geodesic is not built: the geodesic guide needs GeodisTK, which is not available; see --geodesic_guide "
                                  "for this project's own definition of it")
    if getattr(args, "fp_sample", False):
        raise NotImplementedError("--fp_sample is not built: it samples clicks from the false positives of an earlier run's predictions")
    if float(getattr(args, "sample_neg", 0.) or 0.) > 0:
        raise NotImplementedError("--sample_neg > 0 is not built: it samples patches from the false positives of an earlier run's predictions")
    if getattr(args, "downsampling", False):
        raise NotImplementedError("--downsampling is not built: the resident store holds the slices at full resolution")
    if getattr(args, "use_context", False):
        raise NotImplementedError("--use_context is not built for `liver_inter` (the histogram context is `liver`'s, entry.main_g)")


def check_values(args):
    """The value checks of the group; returns the object label."""
    c = int(getattr(args, "im_channel", 3))
    if c < 1 or c % 2 == 0 or c > MAX_CHANNELS:
        raise ValueError("--im_channel must be odd and at most {} (the slices cz - C/2 .. cz + C/2), got {}".format(MAX_CHANNELS, c))
    if int(getattr(args, "guide_channel", 2)) not in (1, 2):
        raise ValueError("--guide_channel must be 1 or 2, got {}".format(args.guide_channel))
    if getattr(args, "local_enhance", False) and not float(getattr(args, "stddev", 3.)) > 0:
        raise ValueError("--stddev must be > 0, got {}".format(args.stddev))
    if float(getattr(args, "noise_scale", 0.)) < 0:
        raise ValueError("--noise_scale must be >= 0, got {}".format(args.noise_scale))
    if getattr(args, "geodesic_guide", False) and not getattr(args, "use_spatial", False):
        raise ValueError("--geodesic_guide needs --use_spatial: it chooses the kind of guide the clicks are rendered into")
    return object_label(args.classes)


def check_args(args):
    """Refuses what is not built, naming the flag; returns the object label."""
    refuse_unbuilt_flags(args)
    mode = getattr(args, "mode", "train")
    if mode != "train":
        raise NotImplementedError("`liver_inter` serves --mode train with online evaluation, got --mode {}: the interactive "
                                  "offline evaluator (evaluators/evaluator_nf.py) is not built yet".format(mode))
    return check_values(args)


def draw_click_tab(rng, bs, max_clicks=CLICKS[3]):
    """The draws `unetk_lits_clicks` takes, uint32 [bs, 12] (include/unetk.h): n_fg = randint(1, N) and n_bg = randint(0, N)
    (inter_simulation :387), the background strategy -- 1 if a uniform draw exceeds 0.5, else 3 (gen_kernel :555-558) -- and
    one 32-bit draw per possible click (np.random.choice: rank = (draw * count) >> 32)."""
    tab = np.zeros((bs, _abi.LITS_CLICK_TAB_COLS), dtype=np.uint32)
    tab[:, 0] = rng.integers(1, max_clicks, bs)
    tab[:, 1] = rng.integers(0, max_clicks, bs)
    tab[:, 2] = np.where(rng.random(bs) > 0.5, 1, 3)
    tab[:, 4:12] = rng.integers(0, 1 << 32, (bs, 8), dtype=np.uint64).astype(np.uint32)
    return tab


def check_status(status, what):
    """Read the kernels' status word (one small device -> host copy: call it where the host synchronises anyway) and raise
    on any bit: each one is a table this module built wrongly, and each would otherwise only show as a run whose samples
    miss their object."""
    word = int(status.item())
    if word != 0:
        raise RuntimeError("liver_inter ({}): {}".format(what, "; ".join(msg for bit, msg in STATUS_BITS if word & bit)))


def batches(store, sampler, args, obj_label, status=None):
    """(features, labels) device batches for ever: features["images"] f32 [bs, H, W, C], features["names"] the case ids,
    with --use_spatial features["sp_guide"] f32 [bs, H, W, guide_channel]; labels int32 [bs, H, W] in {0, 1}.  Per batch:
    one sampler draw, one pinned upload, then `unetk_lits_pick_voxel`, `unetk_lits_inter_batch`, `unetk_lits_clicks` and
    `unetk_click_guide` -- under --geodesic_guide `unetk_lits_inter_center` and `unetk_click_geodesic` in its place -- on the
    current stream: no host synchronisation.  status: int32 [1] device word, NOT read here."""
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=store.device)
    shape = (sampler.depth_out, sampler.h, sampler.w)
    noise = float(getattr(args, "noise_scale", 0.)) if sampler.training else 0.
    spatial = bool(getattr(args, "use_spatial", False))
    stddev = float(getattr(args, "stddev", 3.)) if getattr(args, "local_enhance", False) else None
    channels = int(getattr(args, "guide_channel", 2))
    geodesic = spatial and bool(getattr(args, "geodesic_guide", False))
    while True:
        b = sampler.draw()
        clicks = draw_click_tab(sampler.rng, sampler.bs)
        seed = int(sampler.rng.integers(0, 1 << 32))
        tab, ctab = lits.upload_pinned([sampler.table(b), clicks.view(np.int32)], store.device)
        if sampler.force:
            ops.lits_pick_voxels(store.lb, tab, obj_label, status, lits.LB_SCALE)
        images, labels = ops.lits_inter_batch(store.im, store.lb, tab, shape, sampler.training, status, obj_label, noise, seed,
                                              lits.IM_SCALE, lits.LB_SCALE)
        feats = {"images": images, "names": torch.from_numpy(b["pid"])}
        if spatial:
            pts, cnt = ops.lits_clicks(store.lb, tab, ctab, status, obj_label, CLICKS, lits.LB_SCALE)
            if geodesic:
                base = ops.lits_inter_center(store.im, tab, shape, status, lits.IM_SCALE)
                feats["sp_guide"] = ops.click_geodesic(tab, base, pts, cnt, shape[1:], channels, status=status,
                                                       src_hw=store.im.shape[1:])
            else:
                feats["sp_guide"] = ops.click_guide(tab, pts, cnt, shape[1:], store.im.shape[1:], channels, stddev)
        yield feats, labels


def input_fn(mode, params):
    """input_pipeline_g_simply.py:415-426 for the modes train / eval_online on LiTS; the resident store, the k-fold split
    and the `params` cache keys are `lits.input_fn`'s.  Training: generator seeded seed + 1000 * rank.  eval_online: zoom
    1.125, no flips, gamma or noise, and a rank-independent generator seeded seed + 500 that is re-created for every
    evaluation, so each epoch scores the same --eval_num_batches_per_epoch batches with the same clicks (the reference
    reseeds with 1234, :592).  params[("lits_inter_status", mode == "train")] is the kernels' status word of that stream;
    every evaluation checks both (check_status)."""
    args = params["args"]
    if mode not in ("train", "eval_online"):
        raise ValueError("lits_inter.input_fn handles the modes `train` and `eval_online`, got {}".format(mode))
    obj_label = check_args(args)
    root = params["lits_root"]
    device = params.get("device", torch.device("cuda", torch.cuda.current_device()))
    key = ("lits_store", mode == "train")
    if key not in params:
        cases = lits.collect_datasets(root, args.test_fold, "train" if mode == "train" else "val",
                                      filter_tumor_size=getattr(args, "filter_size", 0))
        params[key] = (lits.SliceStore(root, cases, device, strategy=params.get("strategy")), cases)
    store, cases = params[key]
    if len(cases) == 0:
        raise ValueError("No valid dataset found!")
    ckey = ("lits3d_counts", mode == "train", obj_label)
    if ckey not in params:
        params[ckey] = lits3d.forced_counts(store, obj_label)
    bs = distribution_utils.per_device_batch_size(args.batch_size, args.num_gpus)
    shape = (int(args.im_channel), int(args.im_height), int(args.im_width))
    base_seed = int(getattr(args, "seed", 1234) or 1234)
    training = mode == "train"
    seed = base_seed + 1000 * int(params.get("rank", 0)) if training else base_seed + 500
    sampler = lits3d.PatchSampler(cases, store.offset, params[ckey], bs, shape, store.im.shape[1:],
                                  tumor_percent=getattr(args, "tumor_percent", 0.5), zoom_scale=getattr(args, "zoom_scale", (1., 1.25)),
                                  random_flip=int(getattr(args, "random_flip", 0) or 0) & 3, training=training, seed=seed)
    skey = ("lits_inter_status", training)
    if skey not in params:
        params[skey] = torch.zeros(1, dtype=torch.int32, device=store.device)
    gen = batches(store, sampler, args, obj_label, params[skey])
    if training:
        return gen
    n = int(getattr(args, "eval_num_batches_per_epoch", 100))

    def evaluation():
        if ("lits_inter_status", True) in params:
            check_status(params[("lits_inter_status", True)], "training batches")
        for _ in range(n):
            yield next(gen)
        check_status(params[skey], "eval_online batches")
    return evaluation()


def input_fn_eval(mode, params):
    """Offline evaluation is not built: check_args raises the documented error for every mode but `train`."""
    check_args(params["args"])
    raise NotImplementedError("`liver_inter` serves --mode train with online evaluation, got --mode {}".format(mode))
