"""LiTS training input pipeline for UNet3D: 3-D patches cropped, z-scored, resized, flipped and gamma-augmented on the
device from the resident slice store.

The reference has no LiTS 3-D training pipeline (only DataLoader/Liver/preprocess_3d.py, a one-off resampler).  The
semantics here are those of its 3-D pipeline for the NF data, the volumes are the LiTS cases of `data/lits.SliceStore`:
  * DataLoader/NF/input_pipeline_3d.py:544-604 `gen_batch` -> `PatchSampler` (which cases, which centres, zoom, and the
    draws the reference leaves to TensorFlow: flip coins and gamma);
  * :352-407 `data_processing` (without the use_spatial / cascade branches), DataLoader/misc.py:132-143 `volume_crop`,
    utils/image_ops.py:241 `random_flip`, :339-354 `augment_gamma` -> `unetk_lits_patch3d` (csrc/lits3d.hip).
TensorFlow does not run here: the arithmetic is pinned by the float64 restatement in tests/lits3d_ref.py, which cites the
same lines ("parity unpinned").

A batch costs the host one vectorised sampler draw and ONE pinned upload of the int32 sample table; the centre of a
forced-class sample is picked on the device (`unetk_lits_pick_voxel`) from a (slice, rank) pair, so no voxel position
table exists anywhere and nothing synchronises the host with the device.

Two deviations from the literal reference arithmetic: a case shallower than --im_depth is cropped from slice 0 and padded
with zero slices (the reference would index with a negative start), and a patch without a single non-zero voxel is all
zeros (TensorFlow's moments of an empty tensor are NaN).

With --use_spatial the batches carry `sp_guide`: the clicks of :258-324 `inter_simulation` as :474-504
`gen_kernel` calls it are simulated on the device from per-sample draws made here (`lits_inter.draw_click_tab`, drawn after
the sampler's draw so that an unguided run consumes its generator exactly as without the feature) -> `unetk_lits3d_clicks`;
:364-398 with utils/image_ops.py:437-472 `create_spatial_guide_3d` -> `unetk_click_guide3d`.  The object the clicks are
simulated on is the sampler's forced class (stored label >= fg_label); the restatement is tests/lits3d_clicks_ref.py.

With --random_rotate DEG (not a reference flag) training patches are turned in the plane: the sampler draws an
angle per sample AFTER every other draw of the batch, writes its sin / cos into columns 13 / 14 of the table, and the batches
go through `unetk_lits_patch3d_rot` and `unetk_click_guide3d_rot`; the restatement is tests/lits3d_rotate_ref.py.  Evaluation
never rotates.

With --random_deform PX (not a reference flag) training patches are deformed elastically in the plane: after
the rotation draw the sampler draws, per sample, a coin and a lattice of (G + 3)^2 control displacements from U(-PX, PX) for
each of dy and dx (--deform_grid G cells per axis, a uniform cubic B-spline).  Column 15 of the table marks the deformed rows,
the lattices ride in the batch's one upload, and the batches go through `unetk_lits_patch3d_warp` and
`unetk_click_guide3d_warp`, which serve rotation too; the restatement is tests/lits3d_deform_ref.py.  Evaluation never deforms.

With --slice_prior boundary | binary (the reference's --use_cascade [--cascade_binary] without --use_2d,
:505-533 gen_kernel and :411-471 data_processing_2c) a guided run feeds a second IMAGE channel: the object on the slice of the
first foreground click -- exp(-dist / 25) of the exact Euclidean distance to its inner boundary, or the mask itself on that
slice.  After `unetk_lits3d_clicks`, `unetk_slice_prior_field` and `unetk_slice_prior_render` follow on the same stream and
features["images"] is [bs, D, H, W, 2] (--im_channel 2); the prior consumes no random draw and the host never sees the click.
Training sees only the boundary pixels inside the crop box, the interactive evaluator (entry/main_eval_3d.py) the whole slice
-- the difference the reference has too.  The restatement is tests/slice_prior_ref.py.

Offline, `input_fn_eval` tiles every case of the validation fold with windows cut as `eval_online` cuts them (window_starts,
eval_tables) for the sliding-window evaluator, `EvaluateVolume.run_3d` (--eval_in_patches).  Two options
of that evaluation live here too: the per-axis Gaussian window tables (window_weights, --eval_window_weight gaussian) and
the box of a saved coarse prediction to which the windows are restricted (prediction_box, --eval_box_from).

--mode infer (`input_fn_infer`) serves the same windows over NIfTI volumes that are not in the store: per file
the voxel block goes into pinned memory (VolumeReader: one thread, one case ahead), is uploaded as it lies in the file, and
`unetk_nii_ingest` writes the store's slices on the device (CaseStore).

With --hard_neg_from DIR (the reference's --sample_neg / --fp_sample of nf_3d, :187-219 load_neg, :559-605
gen_batch, :486-504 gen_kernel, inter_simulation strategy 4) training uses the false positives of an earlier run, mined by
`python -m boxsegliver_amd.data.extract neg3d` into DIR/neg-<PID>.npz: they are expanded into a `neg` plane beside store.lb
(load_neg_plane).  --hard_neg_patches P centres ceil(bs P) rows of every batch on a false-positive voxel
(PatchSampler.draw_hard_neg -> `unetk_lits_pick_voxel_rows`), --hard_neg_clicks draws the background clicks inside the false
positives of the crop (`unetk_lits3d_clicks_neg`).  eval_online never sees the plane; the restatement is tests/hard_neg_ref.py.

With --z_spacing MM (not a reference flag) the D output slices of a patch are MM millimetres apart in every case:
a case of slice spacing sz is cropped cd = int(round((D - 1) MM / sz)) + 1 stored slices deep (crop_depth) and resized along z on
the device.  Nothing is drawn for it; the rows' crop depths ride beside the table in the batch's one upload and the batches go
through `unetk_lits_patch3d_z`, the windows of the offline evaluation and of --mode infer are cd slices deep and come back through
`unetk_eval3d_accumulate_z` / `_wz`.  Clicks, rotation and deformation are refused with it; the restatement is
tests/lits3d_zspace_ref.py."""
import math
from pathlib import Path

import numpy as np
import torch

from .. import _abi, ops
from ..utils import distribution_utils
from . import flagsets, lits

EVAL_ZOOM = 1.125                  # gen_batch(train=False): zoom = (1.125, 1.125)   (input_pipeline_3d.py:570-572)
GAMMA_RANGE = (0.7, 1.5)           # data_processing :405
GAMMA_P = 0.3
LABEL_MAPS = (("Liver",), ("Liver", "Tumor"))
WINDOW_WEIGHTS = ("uniform", "gaussian")
MIN_WINDOW_WEIGHT = 1e-30          # the smallest weight of a window, gz[0] * gy[0] * gx[0] in float32, may not fall below this
DEFAULT_BOX_MARGIN = (0, 25, 25)   # (z, y, x): padding_z / padding of the 2-D --eval_in_patches (lits.get_dataset_for_eval_patches)
CLICKS = (3, 10, 40, 5)            # gen_kernel :492-503: margin, step, N; d = 40 for the background band
DEFAULT_STDDEV = (1.0, 3.0, 3.0)   # --stddev of nf_3d: (z, y, x)
STATUS_BITS = ((1, "unetk_lits_pick_voxel: a forced sample's rank was beyond the forced-class count of its slice; the per-slice "
                   "counts do not match the resident store"),
               (2, "unetk_lits_pick_voxel_rows: that rank was a hard-negative row's, beyond the false-positive count of its slice "
                   "of the `neg` plane; the per-slice counts of --hard_neg_from do not match the plane"),
               (4, "unetk_lits3d_clicks: a row of click draws was out of range"))
(COL_BASE, COL_DEPTH, COL_CZ, COL_CY, COL_CX, COL_CH, COL_CW, COL_FLIP_LR, COL_FLIP_UD, COL_FLIP_FB, COL_GAMMA, COL_FORCED,
 COL_K) = range(13)
COL_SIN, COL_COS = 13, 14          # --random_rotate: float bits, both zero = not rotated
COL_WARP = 15                      # --random_deform: 0 = not deformed, else the row's lattice applies
DEFORM_MAX_GRID = 16               # the _warp entries' largest lattice: G + 3 <= 19 control points per axis
DEFORM_FOLD_CAP = 0.4              # largest control displacement as a share of the control spacing (no folding: 7.3.10)
SLICE_PRIORS = ("off", "boundary", "binary")     # --slice_prior
BOUNDARY_MAX_Z_SCALE = 16          # --boundary_z_scale: the cap of unetk_boundary_weights3d
FORCED_LABEL, FORCED_NEG = 1, 2    # COL_FORCED: the centre is picked on store.lb / on the `neg` plane


def add_arguments(parser, z_spacing=True):
    """The flags of DataLoader/NF/input_pipeline_3d.py:53-67 that apply (names / defaults verbatim, data/flagsets.py) +
    --lits_root and --seed as the 2-D LiTS sub-commands add them.  z_spacing=False: without --z_spacing (the interactive
    evaluator, which needs the clicks the flag refuses)."""
    flagsets.add_arguments(parser, "liver_3d")
    if z_spacing:
        parser.add_argument("--z_spacing", type=float, default=None, metavar="MM",
                            help="--mode train / eval --eval_in_patches / infer: the --im_depth output slices of a patch are MM "
                                 "millimetres apart in every case: int(round((im_depth - 1) * MM / slice spacing)) + 1 stored "
                                 "slices are resized along z; default: im_depth consecutive stored slices")
    parser.add_argument("--lits_root", type=str, default="data/LiTS", help="where png/, meta.json and k_folds.txt live")
    parser.add_argument("--seed", type=int, default=1234)
    parser.add_argument("--eval_overlap", type=float, default=0.5,
                        help="--mode eval --eval_in_patches: overlap of neighbouring windows as a share of the window, in [0, 1)")
    parser.add_argument("--random_rotate", type=float, default=0.0, metavar="DEG",
                        help="--mode train: turn every patch in the plane by an angle from U(-DEG, DEG) degrees; 0 = off")
    parser.add_argument("--rotate_prob", type=float, default=1.0, metavar="P",
                        help="--random_rotate: the probability that a sample is rotated")
    parser.add_argument("--random_deform", type=float, default=0.0, metavar="PX",
                        help="--mode train: deform every patch in the plane by a smooth random field; PX = the largest "
                             "displacement of a control point, in pixels of the patch; 0 = off")
    parser.add_argument("--deform_grid", type=int, default=4, metavar="G",
                        help="--random_deform: control cells across the patch on each in-plane axis, 1..16")
    parser.add_argument("--deform_prob", type=float, default=1.0, metavar="P",
                        help="--random_deform: the probability that a sample is deformed")
    parser.add_argument("--slice_prior", type=str, default="off", choices=SLICE_PRIORS,
                        help="--use_spatial: a second image channel (--im_channel 2) from the object on the slice of the first "
                             "foreground click: boundary = exp(-distance to its inner boundary / 25) (the reference's "
                             "--use_cascade), binary = the mask on that slice (--use_cascade --cascade_binary)")
    parser.add_argument("--boundary_z_scale", type=int, default=1, metavar="K",
                        help="--loss_weight_type boundary: the slice spacing in units of the in-plane spacing, an integer in "
                             "1..{}; the distance to a label interface counts K per slice (the patches are not resampled "
                             "along z)".format(BOUNDARY_MAX_Z_SCALE))
    parser.add_argument("--eval_window_weight", type=str, default="uniform", choices=WINDOW_WEIGHTS,
                        help="--eval_in_patches: how a window's voxels count in the average; gaussian weights its centre")
    parser.add_argument("--eval_window_sigma", type=float, default=0.125,
                        help="gaussian: the standard deviation as a share of the window's extent, per axis")
    parser.add_argument("--eval_box_from", type=str, default=None, metavar="DIR",
                        help="--eval_in_patches: tile only the box of predict-<case>.nii.gz in DIR (a --save_predict output)")
    parser.add_argument("--eval_box_margin", type=int, nargs=3, default=DEFAULT_BOX_MARGIN, metavar=("Z", "Y", "X"),
                        help="voxels the --eval_box_from box is grown by on each side, per axis")
    parser.add_argument("--hard_neg_from", type=str, default=None, metavar="DIR",
                        help="--mode train: the neg-<PID>.npz files of `python -m boxsegliver_amd.data.extract neg3d`, the false "
                             "positives of an earlier run's saved predictions; needs --hard_neg_patches or --hard_neg_clicks")
    parser.add_argument("--hard_neg_patches", type=float, default=0.0, metavar="P",
                        help="--hard_neg_from: ceil(batch_size_per_device * P) samples of every training batch are centred on a "
                             "false-positive voxel (the reference's --sample_neg of nf_3d)")
    parser.add_argument("--hard_neg_clicks", action="store_true",
                        help="--hard_neg_from --use_spatial: background clicks of training are drawn from the false positives "
                             "inside the crop (the reference's --fp_sample of nf_3d)")
    parser.add_argument("--infer_volumes", type=str, nargs="+", default=None, metavar="FILE",
                        help="--mode infer: the NIfTI volumes (.nii / .nii.gz) to segment, instead of the validation fold's")
    parser.add_argument("--infer_dir", type=str, default=None, metavar="DIR",
                        help="--mode infer: segment every *.nii / *.nii.gz of DIR, sorted by name")


Z_SPACING_REFUSED = (       # (is the flag given?, its name, why): each needs z-resampling in a kernel of its own
    (lambda a: (getattr(a, "slice_prior", "off") or "off") != "off", "--slice_prior",
     "the prior's field is built on the crop's stored slices"),
    (lambda a: bool(getattr(a, "hard_neg_clicks", False)), "--hard_neg_clicks", "the clicks are simulated on the crop's stored slices"),
    (lambda a: bool(getattr(a, "use_spatial", False)), "--use_spatial",
     "the clicks and the guide are simulated and rendered on the crop's stored slices"),
    (lambda a: float(getattr(a, "random_rotate", 0.0) or 0.0) > 0.0, "--random_rotate", "the rotated rows have a patch kernel of their own"),
    (lambda a: float(getattr(a, "random_deform", 0.0) or 0.0) > 0.0, "--random_deform", "the deformed rows have a patch kernel of their own"))


def z_spacing(args):
    """--z_spacing -> None (off) or MM > 0, finite.  Refused by name with the flags whose kernels do not resample along z."""
    mm = getattr(args, "z_spacing", None)
    if mm is None:
        return None
    mm = float(mm)
    if not 0.0 < mm < float("inf"):                       # also refuses NaN
        raise ValueError("--z_spacing must be a finite number of millimetres > 0, got {}".format(mm))
    for given, flag, why in Z_SPACING_REFUSED:
        if given(args):
            raise NotImplementedError("--z_spacing with {} is not built: {}, which is not resampled along z".format(flag, why))
    return mm


def crop_depth(depth_out, mm, sz):
    """Stored slices that --im_depth output slices MM millimetres apart span in a case of slice spacing sz:
    int(round((D - 1) * MM / sz)) + 1, at least 1; sz == MM gives D.  Not clamped to the case's depth."""
    return max(int(round((int(depth_out) - 1) * float(mm) / float(sz))) + 1, 1)


def case_spacing(case):
    """The slice spacing of a meta.json case, case["spacing"][0]; missing or not a positive finite number: ValueError naming it."""
    spacing = case.get("spacing") if isinstance(case, dict) else None
    try:
        sz = float(spacing[0])
    except (TypeError, ValueError, IndexError, KeyError):
        sz = float("nan")
    if not 0.0 < sz < float("inf"):
        raise ValueError("--z_spacing: case {} has no positive slice spacing in meta.json (spacing = {!r})".format(
            case.get("PID") if isinstance(case, dict) else case, spacing))
    return sz


def crop_depths(cases, depth_out, mm, src_hw):
    """int32 [len(cases)]: crop_depth per case from its meta.json spacing.  Raises before anything is launched when the deepest
    crop cannot be indexed in 31 bits (max(cd) * src_h * src_w >= 2^31, the kernels' limit)."""
    cd = np.array([crop_depth(depth_out, mm, case_spacing(c)) for c in cases], dtype=np.int64)
    check_crop_limit(cd, src_hw, [c.get("PID") for c in cases])
    return cd.astype(np.int32)


def check_crop_limit(cd, src_hw, names=None):
    cd = np.atleast_1d(np.asarray(cd, dtype=np.int64))
    if len(cd) and int(cd.max()) * int(src_hw[0]) * int(src_hw[1]) >= 1 << 31:
        worst = int(np.argmax(cd))
        raise ValueError("--z_spacing: case {} needs a crop of {} slices of {} x {}, beyond 31-bit indexing (>= 2^31 voxels)".format(
            names[worst] if names is not None else worst, int(cd.max()), int(src_hw[0]), int(src_hw[1])))


def check_args(args):
    mode = getattr(args, "mode", "train")
    z_spacing(args)                                        # first: its refusals name the flag, whatever else is wrong with it
    hard = hard_negatives(args)                          # first: --hard_neg_clicks comes with --use_spatial, refused below
    if hard is not None and mode in ("eval", "infer"):
        raise ValueError("{} serve --mode train, got --mode {}".format(" / ".join(hard["flags"]), mode))
    if mode != "infer" and (getattr(args, "infer_volumes", None) or getattr(args, "infer_dir", None) is not None):
        raise ValueError("--infer_volumes / --infer_dir name the volumes of --mode infer, got --mode {}".format(mode))
    if mode == "infer" and (getattr(args, "slice_prior", "off") or "off") != "off":
        raise NotImplementedError("--mode infer with --slice_prior is not built: a prior needs the clicks of the interactive "
                                  "evaluator, entry/main_eval_3d.py")
    if mode == "infer" and getattr(args, "use_spatial", False):
        raise NotImplementedError("--mode infer with --use_spatial is not built: the sliding-window evaluator has no clicks -- "
                                  "real or simulated clicks per case are the interactive evaluator's job, entry/main_eval_3d.py")
    check_values(args)
    if getattr(args, "use_spatial", False) and getattr(args, "mode", "train") == "eval":
        raise NotImplementedError("--mode eval with --use_spatial is not built: the sliding-window evaluator has no clicks -- real "
                                  "or simulated clicks per case are the interactive evaluator's job, entry/main_eval_3d.py")
    return label_map(args.classes)


def check_values(args):
    """The value checks of the flag group, shared with the interactive evaluator (entry/main_eval_3d.py)."""
    prior = slice_prior(args)
    if prior is None and int(getattr(args, "im_channel", 1)) != 1:
        raise ValueError("the LiTS 3-D patches have one channel, got --im_channel {}".format(args.im_channel))
    if prior is not None and int(getattr(args, "im_channel", 1)) != 2:
        raise ValueError("--slice_prior {} is a second image channel: pass --im_channel 2, got --im_channel {}".format(
            prior, getattr(args, "im_channel", 1)))
    overlap = float(getattr(args, "eval_overlap", 0.5))
    if not 0.0 <= overlap < 1.0:                          # also refuses NaN
        raise ValueError("--eval_overlap must satisfy 0 <= v < 1, got {}".format(overlap))
    weight = getattr(args, "eval_window_weight", "uniform")
    if weight not in WINDOW_WEIGHTS:
        raise ValueError("--eval_window_weight must be one of {}, got {}".format(", ".join(WINDOW_WEIGHTS), weight))
    sigma = float(getattr(args, "eval_window_sigma", 0.125))
    if not sigma > 0.0:                                   # also refuses NaN
        raise ValueError("--eval_window_sigma must be > 0, got {}".format(sigma))
    if weight == "gaussian":
        window_weights((int(args.im_depth), int(args.im_height), int(args.im_width)), sigma)     # refuses an underflow
    margin = getattr(args, "eval_box_margin", DEFAULT_BOX_MARGIN)
    if len(margin) != 3 or any(int(m) < 0 for m in margin):
        raise ValueError("--eval_box_margin takes three voxel counts >= 0 (z y x), got {}".format(list(margin)))
    if margin is not DEFAULT_BOX_MARGIN and getattr(args, "eval_box_from", None) is None:       # argparse keeps the default object
        raise ValueError("--eval_box_margin grows the box of --eval_box_from, which is not given")
    guide_stddev(args)
    deg, _ = rotation(args)
    px, _, _ = deformation(args)
    if prior is not None and (deg > 0.0 or px > 0.0):
        raise ValueError("--slice_prior {} is not served together with --random_rotate > 0 or --random_deform > 0: the field is "
                         "not defined beyond the crop box".format(prior))
    if int(getattr(args, "guide_channel", 2)) not in (1, 2):
        raise ValueError("--guide_channel must be 1 or 2, got {}".format(args.guide_channel))
    boundary_z_scale(args)


def hard_negatives(args):
    """--hard_neg_from / --hard_neg_patches / --hard_neg_clicks -> None without any of them, else dict(directory, patches = P,
    clicks, flags = the ones given).  ValueError naming the flag: a training flag without --hard_neg_from, --hard_neg_from
    without one, --hard_neg_clicks without --use_spatial, P outside [0, 1] (or NaN), and more forced rows than the batch has:
    ceil(bs tumor_percent) + ceil(bs P) > bs."""
    directory = getattr(args, "hard_neg_from", None)
    share = float(getattr(args, "hard_neg_patches", 0.0) or 0.0)
    clicks = bool(getattr(args, "hard_neg_clicks", False))
    if not 0.0 <= share <= 1.0:                           # also refuses NaN
        raise ValueError("--hard_neg_patches must satisfy 0 <= P <= 1, got {}".format(share))
    flags = [name for name, on in (("--hard_neg_from", directory is not None), ("--hard_neg_patches", share > 0.0),
                                   ("--hard_neg_clicks", clicks)) if on]
    if not flags:
        return None
    if directory is None:
        raise ValueError("{} needs --hard_neg_from DIR, the neg-<PID>.npz files of `extract neg3d`".format(flags[0]))
    if len(flags) == 1:
        raise ValueError("--hard_neg_from {} is read by --hard_neg_patches P > 0 or --hard_neg_clicks, and neither is "
                         "given".format(directory))
    if clicks and not getattr(args, "use_spatial", False):
        raise ValueError("--hard_neg_clicks needs --use_spatial: it draws the background clicks of the guide")
    if share > 0.0 and getattr(args, "batch_size", None) is not None:
        bs = distribution_utils.per_device_batch_size(args.batch_size, getattr(args, "num_gpus", 1))
        force = int(math.ceil(bs * float(getattr(args, "tumor_percent", 0.5))))
        force_fp = int(math.ceil(bs * share))
        if force + force_fp > bs:
            raise ValueError("--hard_neg_patches {}: ceil(bs * tumor_percent) + ceil(bs * P) = {} + {} rows are forced, a batch has "
                             "{}".format(share, force, force_fp, bs))
    return dict(directory=directory, patches=share, clicks=clicks, flags=flags)


def boundary_z_scale(args):
    """--boundary_z_scale: 1 <= K <= 16, and K != 1 only with --loss_weight_type boundary (elsewhere it would do nothing)."""
    k = int(getattr(args, "boundary_z_scale", 1))
    if not 1 <= k <= BOUNDARY_MAX_Z_SCALE:
        raise ValueError("--boundary_z_scale must satisfy 1 <= K <= {}, got {}".format(BOUNDARY_MAX_Z_SCALE, k))
    w_type = (getattr(args, "loss_weight_type", "none") or "none").lower()
    if k != 1 and w_type != "boundary":
        raise ValueError("--boundary_z_scale {} scales the distances of --loss_weight_type boundary, got --loss_weight_type "
                         "{}".format(k, w_type))
    return k


def slice_prior(args):
    """--slice_prior -> None (off) | "boundary" | "binary"; a prior needs --use_spatial: the first foreground click names the
    slice."""
    mode = getattr(args, "slice_prior", "off") or "off"
    if mode not in SLICE_PRIORS:
        raise ValueError("--slice_prior must be one of {}, got {}".format(", ".join(SLICE_PRIORS), mode))
    if mode == "off":
        return None
    if not getattr(args, "use_spatial", False):
        raise ValueError("--slice_prior {} needs --use_spatial: the slice is the first foreground click's".format(mode))
    return mode


def rotation(args):
    """(--random_rotate in degrees, --rotate_prob): 0 <= DEG <= 180 and 0 <= P <= 1."""
    deg, prob = float(getattr(args, "random_rotate", 0.0) or 0.0), float(getattr(args, "rotate_prob", 1.0))
    if not 0.0 <= deg <= 180.0:                           # also refuses NaN
        raise ValueError("--random_rotate must satisfy 0 <= DEG <= 180, got {}".format(deg))
    if not 0.0 <= prob <= 1.0:
        raise ValueError("--rotate_prob must satisfy 0 <= P <= 1, got {}".format(prob))
    return deg, prob


def deform_cap(hw, grid):
    """The largest --random_deform for an H x W patch and G cells: 0.4 of the control spacing (min(H, W) - 1) / G.  Both
    displacement components of a cubic B-spline stay below their largest control value, so below 0.4 of the spacing -- under
    the 2-D injectivity bound spacing / 2.046 of Choi & Lee (2000): the deformed patch does not fold."""
    return DEFORM_FOLD_CAP * (min(int(hw[0]), int(hw[1])) - 1) / int(grid)


def deformation(args):
    """(--random_deform in pixels, --deform_grid, --deform_prob): PX finite and 0 <= PX <= deform_cap, 1 <= G <= 16 and
    0 <= P <= 1."""
    px = float(getattr(args, "random_deform", 0.0) or 0.0)
    grid, prob = int(getattr(args, "deform_grid", 4)), float(getattr(args, "deform_prob", 1.0))
    if not 0.0 <= px < float("inf"):                      # also refuses NaN
        raise ValueError("--random_deform must be a finite number of pixels >= 0, got {}".format(px))
    if not 1 <= grid <= DEFORM_MAX_GRID:
        raise ValueError("--deform_grid must satisfy 1 <= G <= {}, got {}".format(DEFORM_MAX_GRID, grid))
    if not 0.0 <= prob <= 1.0:
        raise ValueError("--deform_prob must satisfy 0 <= P <= 1, got {}".format(prob))
    if px > 0.0:
        cap = deform_cap((getattr(args, "im_height"), getattr(args, "im_width")), grid)
        if px > cap:
            raise ValueError("--random_deform {} would let the patch fold: with --deform_grid {} on a {} x {} patch the largest "
                             "allowed value is {!r} (0.4 of the control spacing)".format(px, grid, args.im_height, args.im_width,
                                                                                         cap))
    return px, grid, prob


def guide_stddev(args):
    """--stddev -> (s_z, s_y, s_x), three positive numbers (nf_3d's default 1 3 3)."""
    sd = getattr(args, "stddev", DEFAULT_STDDEV)
    try:
        sd = tuple(float(v) for v in sd)
    except TypeError:
        sd = (float(sd),)
    if len(sd) != 3 or not all(v > 0.0 for v in sd):              # also refuses NaN
        raise ValueError("--stddev takes three positive numbers (z y x), got {}".format(list(sd)))
    return sd


def label_map(classes):
    """--classes -> (lab_max, fg_label), as the 2-D LiTS pipelines map them: `Liver Tumor` keeps the stored labels
    {0, 1, 2} (input_pipeline.py), `Liver` alone clips them to {0, 1}, tumour counting as liver (input_pipeline_li.py:230).
    fg_label is the forced class of the sampler: the tumour when it is a class, else the liver."""
    classes = tuple(classes)
    if classes not in LABEL_MAPS:
        raise ValueError("the LiTS labels serve --classes Liver or --classes Liver Tumor, got {}".format(" ".join(classes)))
    return len(classes), 2 if "Tumor" in classes else 1


def forced_counts(store, fg_label):
    """Forced-class pixels of every slice of the store, int64 [n_slices]: counted on the device, ONE transfer."""
    thr = int(fg_label) * lits.LB_SCALE                  # seg // LB_SCALE >= fg  <=>  seg >= fg * LB_SCALE
    n = store.lb.shape[0]
    if thr > 255:
        return np.zeros(n, dtype=np.int64)
    parts = [(store.lb[c0:c0 + 1024] >= thr).sum(dim=(1, 2)) for c0 in range(0, n, 1024)]
    return torch.cat(parts).cpu().numpy().astype(np.int64)


def load_neg_plane(store, cases, directory):
    """The `neg` plane of hard-negative training: uint8 [n_slices, src_h, src_w] beside store.lb and in its
    encoding -- lits.LB_SCALE on the false-positive voxels of DIR/neg-<PID>.npz, else 0 -- so the kernels read it with label 1.
    Per case the PACKED bits are uploaded (1/8 byte per voxel) and expanded on the device.  A case without a file, or a file of
    another shape than the case, is an error naming both: there is no silent zero plane.  Returns (plane, counts int64
    [n_slices] = the files' per-slice counts), checked ONCE against the plane as forced_counts counts it: one transfer."""
    from . import extract
    n, src_h, src_w = store.lb.shape
    plane = torch.zeros((n, src_h, src_w), dtype=torch.uint8, device=store.device)
    counts = np.zeros(n, dtype=np.int64)
    shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=store.device)         # np.packbits: the first voxel in bit 7
    for case in cases:
        pid, depth = int(case["PID"]), int(case["size"][0])
        path = Path(directory) / "neg-{}.npz".format(pid)
        if not path.exists():
            raise FileNotFoundError("--hard_neg_from: training case {} has no false-positive file {}; run `python -m "
                                    "boxsegliver_amd.data.extract neg3d` over that case's prediction".format(pid, path))
        rec = extract.load_neg(path)
        if rec["shape"] != (depth, src_h, src_w):
            raise ValueError("--hard_neg_from: {} holds a mask of shape {}, case {} has {}".format(path, rec["shape"], pid,
                                                                                                   (depth, src_h, src_w)))
        base, vox = int(store.offset[pid]), depth * src_h * src_w
        bits = torch.from_numpy(rec["bits"]).to(store.device)
        flat = ((bits[:, None] >> shifts[None, :]) & 1).reshape(-1)[:vox]
        plane[base:base + depth] = (flat * lits.LB_SCALE).view(depth, src_h, src_w)
        counts[base:base + depth] = rec["slice_counts"]
    have = forced_counts(type("Plane", (object,), {"lb": plane})(), 1)
    if not np.array_equal(have, counts):
        bad = int(np.flatnonzero(have != counts)[0])
        raise ValueError("--hard_neg_from {}: the slice_counts of the files do not match their masks (store slice {}: {} counted, "
                         "{} recorded)".format(directory, bad, int(have[bad]), int(counts[bad])))
    return plane, counts


def crop_shape(target_hw, zoom):
    """gen_batch :589: (float32 target * python floats).astype(int32) -- a float64 product, truncated."""
    return (np.asarray(target_hw, dtype=np.float32).astype(np.float64) * np.asarray(zoom, dtype=np.float64)).astype(np.int32)


class PatchSampler(object):
    """Which cases, centres, crops, flips and gammas make up a batch -- `gen_batch` (input_pipeline_3d.py:544-604) as one
    vectorised draw per batch on a `numpy.random.Generator` of its own:
      * force = ceil(bs * tumor_percent) cases, without replacement, from the cases that hold forced-class voxels (:565,
        :575), each centred on a uniformly chosen forced-class voxel of the case (:592-593);
      * the other bs - force, without replacement, from the cases not chosen above (:582-583), each centred on a uniform
        (pz, py, px) (:598-600);
      * per sample two zoom factors U(zoom_scale) for y and x, crop = int32(target * zoom) (:589); evaluation: 1.125;
      * training: a coin per flip axis enabled in random_flip (image_ops.py:309-314) and gamma -- with probability 0.3 from
        U(0.7, 1), else from U(1, 1.5) (image_ops.py:344-346 as data_processing :405 calls it).
      * training with random_rotate > 0 (not in the reference): a draw of its own, `draw_rotation`, made after
        all of the above (and after a guided run's click draws) -- a coin with probability rotate_prob and an angle from
        U(-random_rotate, random_rotate) degrees per sample.
      * training with random_deform > 0 (not in the reference): `draw_deform`, made after `draw_rotation` --
        a coin with probability deform_prob and 2 (G + 3)^2 control displacements from U(-random_deform, random_deform) per sample.
    A forced-class voxel is chosen WITHOUT a position table: `slice_counts` (forced-class pixels of every store slice, see
    forced_counts) is cumulated once; a rank below the case's total is drawn, searchsorted on the cumulative counts gives
    the slice z and the rank k inside it, and `unetk_lits_pick_voxel` turns (z, k) into (py, px) on the device."""

    def __init__(self, cases, offset, slice_counts, batch_size, shape, src_hw, tumor_percent=0.5, zoom_scale=(1.0, 1.25),
                 random_flip=0, training=True, seed=None, random_rotate=0.0, rotate_prob=1.0, random_deform=0.0, deform_grid=4,
                 deform_prob=1.0, hard_neg_patches=0.0, neg_counts=None, z_spacing=None):
        self.bs = int(batch_size)
        self.deform = float(random_deform or 0.0) if training else 0.0      # pixels; > 0: draw_deform draws
        self.deform_grid = int(deform_grid)
        self.deform_prob = float(deform_prob)
        self.rotate = float(random_rotate or 0.0) if training else 0.0      # degrees; > 0: draw_rotation draws
        self.rotate_prob = float(rotate_prob)
        self.depth_out, self.h, self.w = (int(v) for v in shape)
        self.src_h, self.src_w = int(src_hw[0]), int(src_hw[1])
        self.training = bool(training)
        self.zoom = (float(zoom_scale[0]), float(zoom_scale[1])) if training else (EVAL_ZOOM, EVAL_ZOOM)
        self.flip = int(random_flip or 0) if training else 0
        self.rng = np.random.default_rng(seed)
        cases = list(cases)
        # --z_spacing: the crop depth of every case; no draw depends on it (`crop_depth_rows` reads the batch)
        self.zcrop = crop_depths(cases, shape[0], z_spacing, src_hw) if z_spacing is not None else None
        self.zcrop_max = int(self.zcrop.max()) if self.zcrop is not None and len(self.zcrop) else 0
        self.pid = np.array([int(c["PID"]) for c in cases], dtype=np.int64)
        self.depth = np.array([int(c["size"][0]) for c in cases], dtype=np.int64)
        self.base = np.array([int(offset[int(p)]) for p in self.pid], dtype=np.int64)
        counts = np.asarray(slice_counts, dtype=np.int64)
        self.cum = np.concatenate(([0], np.cumsum(counts)))                     # cum[s] = forced-class pixels before store slice s
        self.case_total = self.cum[self.base + self.depth] - self.cum[self.base]
        self.fg_cases = np.flatnonzero(self.case_total > 0)
        self.force = int(math.ceil(self.bs * float(tumor_percent)))
        if self.force > len(self.fg_cases):
            raise ValueError("too few cases with forced-class voxels: ceil(batch_size * tumor_percent) = {} are drawn without "
                             "replacement, {} of the {} cases have any".format(self.force, len(self.fg_cases), len(cases)))
        if self.bs - self.force > len(cases) - self.force:
            raise ValueError("too few cases: the {} samples beside the forced ones are drawn without replacement from the "
                             "{} other cases".format(self.bs - self.force, len(cases) - self.force))
        # --hard_neg_patches (training only): rows [force, force + force_fp) are re-targeted by draw_hard_neg
        self.force_fp = int(math.ceil(self.bs * float(hard_neg_patches or 0.0))) if training else 0
        if self.force_fp:
            if neg_counts is None:
                raise ValueError("--hard_neg_patches needs the per-slice counts of the `neg` plane")
            if self.force + self.force_fp > self.bs:
                raise ValueError("--hard_neg_patches: ceil(bs * tumor_percent) + ceil(bs * P) = {} + {} rows are forced, a batch "
                                 "has {}".format(self.force, self.force_fp, self.bs))
            if self.force_fp > len(self.fg_cases):
                raise ValueError("--hard_neg_patches: too few cases with forced-class voxels: {} are drawn without replacement, "
                                 "{} have any".format(self.force_fp, len(self.fg_cases)))
            self.neg_cum = np.concatenate(([0], np.cumsum(np.asarray(neg_counts, dtype=np.int64))))
            if len(self.neg_cum) != len(self.cum):
                raise ValueError("the `neg` plane has {} slices, the store {}".format(len(self.neg_cum) - 1, len(self.cum) - 1))
            self.neg_total = self.neg_cum[self.base + self.depth] - self.neg_cum[self.base]

    def locate(self, case, rank):
        """Rank `rank` (< case_total) among the forced-class voxels of case index `case` -> (z within the case, k within
        slice z), element-wise, through the cumulative slice counts."""
        return self._locate(self.cum, case, rank)

    def _locate(self, cum, case, rank):
        case, rank = np.asarray(case, dtype=np.int64), np.asarray(rank, dtype=np.int64)
        target = cum[self.base[case]] + rank
        s = np.searchsorted(cum, target, side="right") - 1                      # the store slice holding that voxel
        return s - self.base[case], target - cum[s]

    def locate_neg(self, case, rank):
        """`locate` on the `neg` plane: rank (< neg_total) among the false-positive voxels of case index `case` -> (z, k)."""
        return self._locate(self.neg_cum, case, rank)

    def draw(self):
        """One batch: dict(case [bs] index into the case list, pid, forced [bs] bool, center [bs, 3] = (z, y, x) with (y, x)
        undefined (0) on forced samples, k [bs], crop [bs, 2], flips [bs, 3] = (left/right, up/down, front/back), gamma [bs])."""
        bs, rng, force = self.bs, self.rng, self.force
        nf = rng.choice(self.fg_cases, size=force, replace=False) if force else np.zeros(0, dtype=np.int64)
        others = np.setdiff1d(np.arange(len(self.pid)), nf)
        rem = rng.choice(others, size=bs - force, replace=False) if bs > force else np.zeros(0, dtype=np.int64)
        case = np.concatenate([nf, rem]).astype(np.int64)
        forced = np.arange(bs) < force
        crop = crop_shape([self.h, self.w], rng.uniform(self.zoom[0], self.zoom[1], (bs, 2)))
        center = np.zeros((bs, 3), dtype=np.int64)
        k = np.zeros(bs, dtype=np.int64)
        if force:
            center[:force, 0], k[:force] = self.locate(nf, rng.integers(0, self.case_total[nf]))
        u = rng.random((bs, 3))
        uniform = np.floor(u * np.stack([self.depth[case], np.full(bs, self.src_h), np.full(bs, self.src_w)], axis=1)).astype(np.int64)
        center[~forced] = uniform[~forced]
        coins = rng.random((bs, 3)) >= 0.5
        flips = coins & np.array([bool(self.flip & 1), bool(self.flip & 2), bool(self.flip & 4)])[None, :]
        low = rng.random(bs) < GAMMA_P
        gamma = np.where(low, rng.uniform(GAMMA_RANGE[0], 1.0, bs), rng.uniform(1.0, GAMMA_RANGE[1], bs))
        if not self.training:
            gamma = np.ones(bs)
        return dict(case=case, pid=self.pid[case], forced=forced, center=center, k=k, crop=crop, flips=flips,
                    gamma=gamma.astype(np.float32))

    def draw_hard_neg(self, b):
        """--hard_neg_patches (gen_batch :577-579, :594-600): re-targets rows [force, force + force_fp) of the
        batch `draw` gave, in place; made right after `draw` and only when force_fp > 0, so a run without the flag consumes its
        generator as before.  force_fp cases from fg_cases without replacement -- a draw of its own, independent of the forced
        one (:578).  A case with false positives: a rank below its total -> (z, k) through the cumulative per-slice counts of
        the plane, forced = FORCED_NEG, and `unetk_lits_pick_voxel_rows` picks (y, x) on the plane.  A case without any: a
        uniform centre in its own extents, forced = 0.  Both draws are made for every row, whichever applies.  b["forced"]
        becomes the int column 11 of the table."""
        fp, rng = self.force_fp, self.rng
        if not fp:
            return b
        rows = np.arange(self.force, self.force + fp)
        case = rng.choice(self.fg_cases, size=fp, replace=False).astype(np.int64)
        total = self.neg_total[case]
        rank = rng.integers(0, np.maximum(total, 1))
        u = rng.random((fp, 3))
        uniform = np.floor(u * np.stack([self.depth[case], np.full(fp, self.src_h), np.full(fp, self.src_w)], axis=1)).astype(np.int64)
        has = total > 0
        z, k = self.locate_neg(case[has], rank[has])
        forced = np.asarray(b["forced"]).astype(np.int64)
        forced[rows] = np.where(has, FORCED_NEG, 0)
        b["case"][rows], b["pid"][rows] = case, self.pid[case]
        b["center"][rows] = uniform
        b["center"][rows[has], 0] = z
        b["center"][rows[has], 1:] = 0
        b["k"][rows] = 0
        b["k"][rows[has]] = k
        b["forced"] = forced
        return b

    def draw_rotation(self):
        """The rotation draw of one batch, made only when --random_rotate > 0 and AFTER every other draw of
        the batch (`draw`, and the click draws of a guided run), so that a run without the flag consumes its generator as
        before: dict(on [bs] bool with probability rotate_prob, deg [bs] from U(-DEG, DEG)), or None."""
        if not self.rotate > 0.0:
            return None
        on = self.rng.random(self.bs) < self.rotate_prob
        return dict(on=on, deg=self.rng.uniform(-self.rotate, self.rotate, self.bs))

    def draw_deform(self):
        """The deformation draw of one batch, made only when --random_deform > 0 and AFTER `draw_rotation`
        (so after every other draw of the batch): dict(on [bs] bool with probability deform_prob, ctl float32
        [bs, 2, G + 3, G + 3] from U(-PX, PX), component 0 = dy and 1 = dx), or None."""
        if not self.deform > 0.0:
            return None
        on = self.rng.random(self.bs) < self.deform_prob
        g = self.deform_grid + 3
        return dict(on=on, ctl=self.rng.uniform(-self.deform, self.deform, (self.bs, 2, g, g)).astype(np.float32))

    def crop_depth_rows(self, b):
        """--z_spacing: int32 [bs], the crop depth of every row's case, for the batch `draw` (and `draw_hard_neg`) gave; None
        without the flag.  It travels BESIDE the table (all 16 columns are taken) in the batch's one upload and draws nothing."""
        return None if self.zcrop is None else np.ascontiguousarray(self.zcrop[np.asarray(b["case"])], dtype=np.int32)

    def table(self, b=None, rot=None, warp=None):
        """The batch as `unetk_lits_patch3d` takes it: int32 [bs, 16] (include/unetk.h), gamma as float bits.  rot: what
        `draw_rotation` gave -- the `on` rows get sin / cos (float64, cast to float32; float bits) in columns 13 / 14 for
        `unetk_lits_patch3d_rot`, every other row keeps zeros there.  warp: what `draw_deform` gave -- the `on` rows get 1 in
        column 15 for `unetk_lits_patch3d_warp`, which takes warp["ctl"] beside the table.  Without b the sampler draws the
        batch and the rotation (a deformation comes with its lattices, so its draw is the caller's)."""
        if b is None:
            b, rot = self.draw(), self.draw_rotation()
        tab = np.zeros((self.bs, _abi.LITS3D_TAB_COLS), dtype=np.int32)
        if warp is not None:
            tab[:, COL_WARP] = np.asarray(warp["on"], dtype=bool)
        if rot is not None:
            rad = np.deg2rad(np.asarray(rot["deg"], dtype=np.float64))
            on = np.asarray(rot["on"], dtype=bool)
            tab[on, COL_SIN] = np.sin(rad).astype(np.float32).view(np.int32)[on]
            tab[on, COL_COS] = np.cos(rad).astype(np.float32).view(np.int32)[on]
        tab[:, COL_BASE] = self.base[b["case"]]
        tab[:, COL_DEPTH] = self.depth[b["case"]]
        tab[:, COL_CZ:COL_CX + 1] = b["center"]
        tab[:, COL_CH:COL_CW + 1] = b["crop"]
        tab[:, COL_FLIP_LR:COL_FLIP_FB + 1] = b["flips"]
        tab[:, COL_GAMMA] = np.ascontiguousarray(b["gamma"], dtype=np.float32).view(np.int32)
        tab[:, COL_FORCED] = b["forced"]
        tab[:, COL_K] = b["k"]
        return tab


def check_status(status, what):
    """Read the pick kernel's status word (one small device -> host copy: call it where the host synchronises anyway) and
    raise if a forced sample's rank lay beyond its slice's count -- per-slice counts that do not match the store.  Such a
    sample is centred on (0, 0), so without this check the bug would only show as a run that never sees its forced class."""
    word = int(status.item())
    if word != 0:
        raise RuntimeError("liver_3d ({}): {}".format(what, "; ".join(msg for bit, msg in STATUS_BITS if word & bit) or
                                                      "status word {}".format(word)))


def batches(store, sampler, shape, lab_max, fg_label, status=None, guide=None, prior=None, neg_clicks=False):
    """(features, labels) device batches for ever: features["images"] f32 [bs, D, H, W, 1], features["names"] the case ids,
    labels int32 [bs, D, H, W].  Per batch: one sampler draw, one pinned upload, then `unetk_lits_pick_voxel` (forced
    samples' centres, in the device table) and `unetk_lits_patch3d` on the current stream -- no host synchronisation.
    status: int32 [1] device word that collects the kernels' bits (STATUS_BITS); it is NOT read here (that would
    synchronise): the owner reads it with `check_status` at a point that synchronises anyway (input_fn: every evaluation).
    guide: None, or dict(channels, stddev) for --use_spatial (stddev None: the Euclidean guide): the click draws are made
    after the sampler's and ride in the same upload, `unetk_lits3d_clicks` and `unetk_click_guide3d` follow on the same
    stream and features["sp_guide"] is f32 [bs, D, H, W, channels].
    prior: None, or "boundary" / "binary" for --slice_prior (needs guide): `unetk_slice_prior_field` on the clicks just simulated
    and `unetk_slice_prior_render` follow on the same stream, features["images"] is f32 [bs, D, H, W, 2] with channel 0 the
    one-channel patch bit for bit.  No draw, no upload and no synchronisation is added.
    Hard negatives need store.neg, the plane of load_neg_plane: a sampler with force_fp > 0 re-targets rows
    (draw_hard_neg, right after draw) and the centres are picked per plane by `unetk_lits_pick_voxel_rows`; neg_clicks: the
    clicks come from `unetk_lits3d_clicks_neg`.  Without either the calls are exactly those of a run without the flags.
    --z_spacing (a sampler built with z_spacing): the rows' crop depths, int32 [bs], ride beside the table in the
    same upload and the batch goes through `unetk_lits_patch3d_z`; nothing is drawn for it."""
    hard_rows = getattr(sampler, "force_fp", 0) > 0
    if (hard_rows or neg_clicks) and getattr(store, "neg", None) is None:
        raise ValueError("hard negatives need the store's `neg` plane (load_neg_plane)")
    if neg_clicks and guide is None:
        raise ValueError("--hard_neg_clicks needs the simulated clicks of a guided run")
    if prior is not None and guide is None:
        raise ValueError("a slice prior needs the simulated clicks of a guided run")
    zspace = getattr(sampler, "zcrop", None) is not None
    if zspace and (guide is not None or sampler.rotate > 0.0 or sampler.deform > 0.0):
        raise ValueError("--z_spacing is not served together with --use_spatial, --random_rotate or --random_deform")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=store.device)
    while True:
        b = sampler.draw()
        if hard_rows:
            b = sampler.draw_hard_neg(b)
        parts = []
        if guide is not None:
            from . import lits_inter
            parts.append(lits_inter.draw_click_tab(sampler.rng, sampler.bs, CLICKS[3]).view(np.int32))
        rot = sampler.draw_rotation()
        deform = sampler.draw_deform()                       # --random_deform: the last draw; the lattices ride in the same upload
        if deform is not None:
            parts.append(deform["ctl"].view(np.int32))
        zrows = sampler.crop_depth_rows(b) if zspace else None                   # --z_spacing: no draw; rides in the same upload
        if zspace:
            parts.insert(0, zrows)
        dev = lits.upload_pinned([sampler.table(b, rot, deform)] + parts, store.device)
        tab, ctab = dev[0], dev[1] if guide is not None else None
        warp, grid = (dev[-1].view(torch.float32), sampler.deform_grid) if deform is not None else (None, 0)
        zkw = dict(zcrop=dev[1], zcrop_max=sampler.zcrop_max) if zspace else {}
        if hard_rows:                                        # one call per plane, each serving its own rows
            if sampler.force:
                ops.lits_pick_voxel_rows(store.lb, tab, FORCED_LABEL, status, fg_label, lits.LB_SCALE)
            ops.lits_pick_voxel_rows(store.neg, tab, FORCED_NEG, status, 1, lits.LB_SCALE)
        elif sampler.force:
            ops.lits_pick_voxels(store.lb, tab, fg_label, status, lits.LB_SCALE)
        rotate = sampler.rotate > 0.0                        # --random_rotate: the _rot entries, which read the table's (sin, cos)
        images, labels = ops.lits_patch3d(store.im, store.lb, tab, shape, sampler.training, lab_max, lits.IM_SCALE, lits.LB_SCALE,
                                          rotate=rotate, warp=warp, grid=grid, **zkw)
        feats = {"images": images, "names": torch.from_numpy(b["pid"])}
        if guide is not None:
            pts, cnt = ops.lits3d_clicks(store.lb, tab, ctab, shape, status, fg_label, CLICKS, lits.LB_SCALE,
                                         neg_slices=store.neg if neg_clicks else None)
            feats["sp_guide"] = ops.click_guide3d(tab, pts, cnt, shape, store.im.shape[1:], guide["channels"], guide["stddev"],
                                                  rotate=rotate, warp=warp, grid=grid)
            if prior is not None:
                field, z0 = ops.slice_prior_field(store.lb, tab, pts, cnt, shape, fg_label, prior, lab_scale=lits.LB_SCALE)
                feats["images"] = ops.slice_prior_render(tab, images, field, z0, shape, store.im.shape[1:], prior)
        yield feats, labels


def guide_config(args):
    """None without --use_spatial, else what `batches` renders: dict(channels = --guide_channel, stddev = --stddev with
    --local_enhance, None for the Euclidean guide)."""
    if not getattr(args, "use_spatial", False):
        return None
    return dict(channels=int(getattr(args, "guide_channel", 2)),
                stddev=guide_stddev(args) if getattr(args, "local_enhance", False) else None)


def input_fn(mode, params):
    """input_pipeline_3d.py:336-343 for the modes train / eval_online on LiTS; the resident store, the k-fold split and the
    `params` cache keys are `lits.input_fn`'s.  Training: generator seeded seed + 1000 * rank.  eval_online: zoom 1.125, no
    flips, no gamma, and a rank-independent generator seeded seed + 500 that is re-created for every evaluation, so each
    epoch scores the same --eval_num_batches_per_epoch batches (the reference reseeds with 1234 when it builds the
    generator, :571).  params[("lits3d_status", mode == "train")] is the pick kernel's status word of that stream; every
    evaluation checks both (check_status), a trainer without online evaluation can check the training one itself."""
    args = params["args"]
    if mode not in ("train", "eval_online"):
        raise ValueError("lits3d.input_fn handles the modes `train` and `eval_online`, got {}".format(mode))
    lab_max, fg_label = check_args(args)
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
    ckey = ("lits3d_counts", mode == "train", fg_label)
    if ckey not in params:
        params[ckey] = forced_counts(store, fg_label)
    bs = distribution_utils.per_device_batch_size(args.batch_size, args.num_gpus)
    shape = (int(args.im_depth), int(args.im_height), int(args.im_width))
    base_seed = int(getattr(args, "seed", 1234) or 1234)
    training = mode == "train"
    seed = base_seed + 1000 * int(params.get("rank", 0)) if training else base_seed + 500
    deg, prob = rotation(args)                             # only `train` rotates: the sampler drops it for eval_online
    px, grid, dprob = deformation(args)                    # likewise
    hard = hard_negatives(args) if training else None      # eval_online never uses the plane (gen_batch: `train and ...`)
    if hard is not None and getattr(store, "neg", None) is None:
        store.neg, params[("lits3d_neg_counts",)] = load_neg_plane(store, cases, hard["directory"])
    sampler = PatchSampler(cases, store.offset, params[ckey], bs, shape, store.im.shape[1:],
                           hard_neg_patches=hard["patches"] if hard is not None else 0.0,
                           neg_counts=params[("lits3d_neg_counts",)] if hard is not None else None,
                           tumor_percent=getattr(args, "tumor_percent", 0.5), zoom_scale=getattr(args, "zoom_scale", (1., 1.25)),
                           random_flip=getattr(args, "random_flip", 0), training=training, seed=seed, random_rotate=deg,
                           rotate_prob=prob, random_deform=px, deform_grid=grid, deform_prob=dprob, z_spacing=z_spacing(args))
    # the pick kernel's status words live in `params` (one per mode) so that they outlast the generators: params[("lits3d_status",
    # True)] is the training stream's.  An evaluation synchronises anyway, so both are read there: the training word when
    # the evaluation starts, the evaluation's own after its last batch.
    skey = ("lits3d_status", training)
    if skey not in params:
        params[skey] = torch.zeros(1, dtype=torch.int32, device=store.device)
    gen = batches(store, sampler, shape, lab_max, fg_label, params[skey], guide_config(args), slice_prior(args),
                  neg_clicks=hard is not None and hard["clicks"])
    if training:
        return gen
    n = int(getattr(args, "eval_num_batches_per_epoch", 100))

    def evaluation():
        if ("lits3d_status", True) in params:
            check_status(params[("lits3d_status", True)], "training batches")
        for _ in range(n):
            yield next(gen)
        check_status(params[skey], "eval_online batches")
    return evaluation()


# ------------------------------------------------------------------------------------------------- whole-volume evaluation
def window_starts(extent, window, overlap):
    """Where the windows of one axis start (evaluators/evaluator_nf.py:194-257 walks its patches the same way): every
    step = max(int(window * (1 - overlap)), 1) while the window fits, plus one window aligned with the end when the last one
    stops short of it; an axis no longer than the window has the one start 0."""
    extent, window = int(extent), int(window)
    if extent <= window:
        return [0]
    step = max(int(window * (1 - float(overlap))), 1)
    starts = list(range(0, extent - window + 1, step))
    if starts[-1] + window != extent:
        starts.append(extent - window)
    return starts


def mirror_variants(args):
    """The flip sets (left/right, up/down, front/back) of the mirror test-time augmentation, entry/main_eval_3d.py:246-287
    literally: the plain window, and with --eval_mirror every m in 1..7 with (random_flip & m) > 0, bit 0 = left/right,
    bit 1 = up/down, bit 2 = front/back -- so `--random_flip 1` also runs m = 3, 5, 7, a quirk kept as
    evaluator_liver.mirror_plan keeps the 2-D one."""
    variants = [0]
    if getattr(args, "eval_mirror", False):
        rf = int(getattr(args, "random_flip", 0) or 0)
        variants += [m for m in range(1, 8) if (rf & m) > 0]
    return [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in variants]


def eval_windows(src_hw, shape, cd=None):
    """(D, ch, cw): a window's extent in the case -- im_depth slices (fewer exist in a shallower case) and the
    `eval_online` crop int32((H, W) * EVAL_ZOOM) clamped to the slice, as the kernels' crop box clamps it.  cd: the case's crop
    depth with --z_spacing (crop_depth), which takes the place of D: (cd, ch, cw)."""
    ch, cw = (int(v) for v in crop_shape(shape[1:], (EVAL_ZOOM, EVAL_ZOOM)))
    return int(shape[0] if cd is None else cd), min(max(ch, 1), int(src_hw[0])), min(max(cw, 1), int(src_hw[1]))


def window_weights(shape, sigma):
    """--eval_window_weight gaussian: (gz [D], gy [H], gx [W]) float32, the weight of a window's voxel per axis.  Axis of n
    voxels: exp(-((i - (n - 1) / 2) / (sigma n))^2 / 2) in float64, divided by its maximum, rounded to float32; built as
    one half and its mirror, so g[i] == g[n - 1 - i] bit for bit.  The smallest weight of a window, gz[0] gy[0] gx[0]
    formed in float32, must stay >= MIN_WINDOW_WEIGHT: a voxel that only such corners cover would otherwise carry a sum
    and a weight of 0 (or denormals) and count as not covered."""
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError("--eval_window_sigma must be > 0, got {}".format(sigma))
    tables = []
    for n in (int(v) for v in shape):
        i = np.arange((n + 1) // 2, dtype=np.float64)
        half = np.exp(-0.5 * ((i - (n - 1) / 2.0) / (sigma * n)) ** 2)
        half = (half / half.max()).astype(np.float32)
        tables.append(np.concatenate([half, half[:n // 2][::-1]]))
    smallest = np.float32(tables[0][0] * tables[1][0]) * tables[2][0]
    if not smallest >= np.float32(MIN_WINDOW_WEIGHT):
        raise ValueError("--eval_window_sigma {} is too small for windows of {} x {} x {}: the corner weight {:.3g} underflows "
                         "(it must be >= {:g})".format(sigma, shape[0], shape[1], shape[2], float(smallest), MIN_WINDOW_WEIGHT))
    return tuple(tables)


def prediction_box(directory, case, depth, src_hw, margin=DEFAULT_BOX_MARGIN, special=None):
    """--eval_box_from: (z0, z1, y0, y1, x0, x1), the box of the foreground of `<directory>/predict-<PID>.nii.gz` (what
    --save_predict writes, voxel for voxel on the case's volume file), grown by margin = (z, y, x) and clamped to the case.
    The file is read with the volume's mirror rule (nii_kits.read_lits("vol"): cases 28..47), so the array lines up with
    the resident store.  A missing file, another shape than (depth, src_h, src_w) or an empty mask raise: there is no
    fallback to the whole volume."""
    from . import nii_kits
    if special is None:
        pid = int(case["PID"]) if isinstance(case, dict) else int(case)
        special = 28 <= pid < 48
    else:                                                  # --mode infer: the case's id and mirror rule are the input file's
        pid = str(case)
    path = Path(directory) / "predict-{}.nii.gz".format(pid)
    if not path.exists():
        raise FileNotFoundError("--eval_box_from: {} does not exist".format(path))
    _, mask = nii_kits.read_nii(path, out_dtype=np.uint8, special=special)
    want = (int(depth), int(src_hw[0]), int(src_hw[1]))
    if tuple(mask.shape) != want:
        raise ValueError("--eval_box_from: {} holds a volume of shape {}, case {} has {}".format(path, tuple(mask.shape), pid, want))
    box = []
    for axis, (extent, grow) in enumerate(zip(want, margin)):
        hit = np.flatnonzero((mask > 0).any(axis=tuple(a for a in range(3) if a != axis)))
        if len(hit) == 0:
            raise ValueError("--eval_box_from: {} predicts nothing, case {} has no box".format(path, pid))
        box += [max(int(hit[0]) - int(grow), 0), min(int(hit[-1]) + 1 + int(grow), extent)]
    return tuple(box)


def box_starts(extent, window, overlap, lo, hi):
    """window_starts for the part [lo, hi) of an axis: the one start 0 on an axis no longer than the window; a part no
    longer than the window gets ONE window centred on it and clamped to the axis; else the part is tiled like an axis of
    its own.  [0, extent) gives window_starts(extent, window, overlap)."""
    extent, window, lo, hi = int(extent), int(window), int(lo), int(hi)
    if extent <= window:
        return [0]
    if hi - lo <= window:
        return [min(max(lo - (window - (hi - lo)) // 2, 0), extent - window)]
    return [lo + s for s in window_starts(hi - lo, window, overlap)]


def eval_tables(case, store, shape, overlap, variants, batch_size, box=None, cd=None):
    """The sample tables (PatchSampler.table's layout, int32 [n, 16]) that tile ONE case with windows, in batches of
    `batch_size` rows, the last one short.  Windows are cut as `eval_online` cuts them (zoom EVAL_ZOOM, no gamma, not
    forced) and cover the whole volume -- not the ground-truth liver box: no label information enters the prediction --
    or, with box = (z0, z1, y0, y1, x0, x1) (prediction_box), that box: box_starts per axis.
    A window that starts at `a` is centred on a + window // 2, from which the kernels' volume_crop clamp gives back `a`.
    Every window is followed by its mirror variants: the same row with the flip columns set.
    cd: the case's crop depth with --z_spacing (crop_depth): the windows are cd stored slices deep, tiled with window_starts(depth,
    cd, overlap), and the rows' crop depths (all cd) go beside each table to the _z entries."""
    pid, depth = int(case["PID"]), int(case["size"][0])
    src_h, src_w = int(store.im.shape[1]), int(store.im.shape[2])
    d, ch, cw = eval_windows((src_h, src_w), shape, cd)
    if box is None:
        box = (0, depth, 0, src_h, 0, src_w)
    elif not (0 <= box[0] < box[1] <= depth and 0 <= box[2] < box[3] <= src_h and 0 <= box[4] < box[5] <= src_w):
        raise ValueError("the box {} is empty or leaves case {} ({} x {} x {})".format(tuple(box), pid, depth, src_h, src_w))
    rows = []
    for z in box_starts(depth, d, overlap, box[0], box[1]):
        for y in box_starts(src_h, ch, overlap, box[2], box[3]):
            for x in box_starts(src_w, cw, overlap, box[4], box[5]):
                for flips in variants:
                    row = np.zeros(_abi.LITS3D_TAB_COLS, dtype=np.int32)
                    row[COL_BASE], row[COL_DEPTH] = int(store.offset[pid]), depth
                    row[COL_CZ:COL_CX + 1] = z + d // 2, y + ch // 2, x + cw // 2
                    row[COL_CH:COL_CW + 1] = ch, cw
                    row[COL_FLIP_LR:COL_FLIP_FB + 1] = flips
                    row[COL_GAMMA] = np.array([1.0], dtype=np.float32).view(np.int32)[0]
                    rows.append(row)
    tab = np.stack(rows)
    bs = max(int(batch_size), 1)
    for i in range(0, len(tab), bs):
        yield tab[i:i + bs]


def table_box(tab, shape, depth, src_hw, cd=None):
    """(z0, z1, y0, y1, x0, x1): the union box of a table's crop boxes inside the case (the voxels
    `unetk_eval3d_accumulate` visits), computed as the kernels' crop box (p3d_box, csrc/lits3d.hip) computes them.  cd: the
    rows' crop depth with --z_spacing, in place of D (p3d_box_z)."""
    tab = np.asarray(tab).astype(np.int64)
    d, depth = int(shape[0] if cd is None else cd), int(depth)
    ch = np.clip(tab[:, COL_CH], 1, int(src_hw[0]))
    cw = np.clip(tab[:, COL_CW], 1, int(src_hw[1]))
    z1 = np.minimum(np.maximum(tab[:, COL_CZ] - d // 2, 0), max(depth - d, 0))
    y1 = np.minimum(np.maximum(tab[:, COL_CY] - ch // 2, 0), int(src_hw[0]) - ch)
    x1 = np.minimum(np.maximum(tab[:, COL_CX] - cw // 2, 0), int(src_hw[1]) - cw)
    return (int(z1.min()), int(min((z1 + d).max(), depth)), int(y1.min()), int((y1 + ch).max()), int(x1.min()),
            int((x1 + cw).max()))


def input_fn_eval(mode, params):
    """Offline evaluation (--mode eval) in sliding windows, --eval_in_patches.  The validation fold is
    loaded into the resident store exactly as input_fn("eval_online") loads it (same cache key).  Per case the generator
    yields its window tables (host int32 [n, 16], eval_tables) and then one end-of-case item
    (None, dict(case, base, depth, store)), which with --eval_box_from also carries `box`, the box the windows were
    restricted to (prediction_box).  Labels never leave the device: the evaluator takes them from store.lb.
    Without the flag: the reference's other way, one forward over the whole case (entry/main_eval_3d.py), which is not built."""
    args = params["args"]
    # NIfTI volumes in, --eval_in_patches implied -- for arguments of --mode infer: the flags of that mode
    # (which volumes, whether labels exist) are the arguments', so a mode that disagrees with them is served by nobody
    if mode == "infer" and getattr(args, "mode", mode) == "infer":
        return input_fn_infer(mode, params)
    if not getattr(args, "eval_in_patches", False):
        raise NotImplementedError("whole-volume 3-D evaluation of UNet3D on LiTS in ONE forward is not built; pass "
                                  "--eval_in_patches for the sliding-window evaluator")
    if mode != "eval":
        raise NotImplementedError("`liver_3d` serves --mode train, --mode eval --eval_in_patches and --mode infer with arguments "
                                  "of that mode, got mode {} with --mode {}".format(mode, getattr(args, "mode", None)))
    check_args(args)
    return _eval_cases(args, params)


def _eval_cases(args, params):
    root = params["lits_root"]
    key = ("lits_store", False)
    if key not in params:
        device = params.get("device") or torch.device("cuda", torch.cuda.current_device())
        cases = lits.collect_datasets(root, args.test_fold, "val", filter_tumor_size=getattr(args, "filter_size", 0))
        params[key] = (lits.SliceStore(root, cases, device, strategy=params.get("strategy")), cases)
    store, cases = params[key]
    if len(cases) == 0:
        raise ValueError("No valid dataset found!")
    cases = cases[int(getattr(args, "eval_skip_num", 0) or 0):]
    if int(getattr(args, "eval_num", -1)) > 0:
        cases = cases[:int(args.eval_num)]
    bs = distribution_utils.per_device_batch_size(args.batch_size, args.num_gpus)
    shape = (int(args.im_depth), int(args.im_height), int(args.im_width))
    variants = mirror_variants(args)
    box_from = getattr(args, "eval_box_from", None)
    mm = z_spacing(args)
    # --z_spacing: every case's crop depth, checked for all of them before the first window is cut
    depths = crop_depths(cases, shape[0], mm, store.im.shape[1:]) if mm is not None else None
    for i, case in enumerate(cases):
        pid, depth = int(case["PID"]), int(case["size"][0])
        end = dict(case=str(pid), base=int(store.offset[pid]), depth=depth, store=store)
        box = None
        if box_from is not None:
            box = end["box"] = prediction_box(box_from, case, depth, store.im.shape[1:], getattr(args, "eval_box_margin", DEFAULT_BOX_MARGIN))
        cd = int(depths[i]) if depths is not None else None
        for tab in eval_tables(case, store, shape, float(getattr(args, "eval_overlap", 0.5)), variants, bs, box, cd=cd):
            yield tab, ({"zcrop": cd} if cd is not None else None)
        yield None, end


# ------------------------------------------------------------------------------------------------- NIfTI volumes in (--mode infer)
NII_SUFFIXES = (".nii.gz", ".nii")


def infer_case_id(path):
    """(id, special) of an input volume: the file name without .nii[.gz]; `volume-<N>` is LiTS case N -- id "<N>", read with
    read_lits's rule (x-mirrored for 28 <= N < 48, lits._load_lits_volume's distinction), so its slices equal the stored ones.
    Any other name is read plainly."""
    import re
    name = Path(path).name
    for suffix in NII_SUFFIXES:
        if name.endswith(suffix):
            name = name[:-len(suffix)]
            break
    else:
        raise ValueError("{}: a .nii or .nii.gz file expected".format(path))
    m = re.fullmatch(r"volume-(\d+)", name)
    if m:
        return str(int(m.group(1))), 28 <= int(m.group(1)) < 48
    return name, False


def infer_files(args, params):
    """The volumes of --mode infer, in order: --infer_volumes as given, then --infer_dir's *.nii / *.nii.gz sorted by name;
    with neither flag the `vol_case` files of the validation fold (meta.json under params["lits_root"], paths relative to
    params["proj_root"]), as the 2-D --mode infer takes them.  A missing file raises FileNotFoundError naming it."""
    volumes, directory = getattr(args, "infer_volumes", None), getattr(args, "infer_dir", None)
    files = [Path(v) for v in (volumes or [])]
    if directory is not None:
        if not Path(directory).is_dir():
            raise FileNotFoundError("--infer_dir: {} is not a directory".format(directory))
        files += sorted((p for p in Path(directory).iterdir() if p.name.endswith(NII_SUFFIXES)), key=lambda p: p.name)
    if not volumes and directory is None:
        cases = lits.collect_datasets(params["lits_root"], args.test_fold, "val", filter_tumor_size=getattr(args, "filter_size", 0))
        for case in cases:
            if not case.get("vol_case"):
                raise ValueError("--mode infer: case {} of meta.json names no vol_case; pass --infer_volumes or "
                                 "--infer_dir".format(case["PID"]))
            files.append(Path(params.get("proj_root", ".")) / case["vol_case"])
    if not files:
        raise ValueError("No valid dataset found!")
    for f in files:
        if not f.exists():
            raise FileNotFoundError("--mode infer: the volume {} does not exist".format(f))
    ids = [infer_case_id(f)[0] for f in files]
    if len(set(ids)) != len(ids):
        raise ValueError("--mode infer: two volumes share a case id (their outputs would share a file name): {}".format(ids))
    return files


def infer_plan(path):
    """What unetk_nii_ingest needs of one file, from its header alone: dict(header, case, special, dtype, file_shape, nbytes,
    trans_bk, flips, shape = (d, h, w)).  Big-endian files, other than 3-D data and oblique affines are refused."""
    from . import nii_kits
    header = nii_kits.load_header(path)
    if header.endian != "<":
        raise ValueError("{}: big-endian NIfTI files are not supported".format(path))
    if len(header.shape) != 3 or min(header.shape) < 1:
        raise ValueError("{}: a 3-D volume expected, the file holds shape {}".format(path, header.shape))
    if header.dtype.name not in ops.NII_INGEST_CODES:
        raise ValueError("{}: unsupported NIfTI datatype {}".format(path, header.dtype))
    case, special = infer_case_id(path)
    try:
        trans_bk, flips = nii_kits.file_orientation(header, special)
    except ValueError as e:
        raise ValueError("{}: {}".format(path, e))
    return dict(header=header, case=case, special=special, dtype=header.dtype, file_shape=tuple(header.shape),
                nbytes=int(np.prod(header.shape)) * header.dtype.itemsize, trans_bk=trans_bk, flips=flips,
                shape=nii_kits.data_shape(header))


def infer_spacing(path, plan):
    """--z_spacing in --mode infer: the slice spacing of an input volume = the pixdim of whichever FILE axis the ingest maps to
    the store's z axis (plan["trans_bk"][i] == 0), not pixdim[3] of a transposed file.  Not a positive finite number: ValueError
    naming the file."""
    axis = [int(a) for a in plan["trans_bk"]].index(0)
    pixdim = tuple(plan["header"].pixdim)
    sz = float(pixdim[axis]) if axis < len(pixdim) else float("nan")
    if not 0.0 < sz < float("inf"):
        raise ValueError("--z_spacing: {} (case {}) has no positive slice spacing: pixdim[{}] = {!r}".format(
            path, plan["case"], axis + 1, pixdim[axis] if axis < len(pixdim) else None))
    return sz


def read_voxel_block(path, header, view):
    """The file's voxel block (what lies behind vox_offset) straight into `view`, a writable byte buffer of exactly the
    block's size; a .gz is inflated with readinto -- no intermediate copy of the volume exists.  Every failure names the file."""
    import zlib
    from . import nii_kits
    view = memoryview(view).cast("B")
    try:
        with nii_kits._open(path, "rb") as f:
            skip = int(header.vox_offset)
            if len(f.read(skip)) != skip:
                raise ValueError("ends inside its header")
            got = 0
            while got < len(view):
                n = f.readinto(view[got:])
                if not n:
                    break
                got += n
            if got == len(view):
                f.read(1)                                  # a .gz whose stream ends here checks its CRC now, not never
        if got != len(view):
            raise ValueError("holds {} of the {} bytes of its voxel block".format(got, len(view)))
    except (OSError, EOFError, ValueError, zlib.error) as e:
        if isinstance(e, FileNotFoundError):
            raise FileNotFoundError("--mode infer: the volume {} does not exist".format(path))
        raise ValueError("{}: {}".format(path, e))


class VolumeReader(object):
    """The host side of --mode infer: header, then the voxel block into one of two staging buffers (pinned on a GPU run, grown
    to the largest case seen).  With ahead=True ONE background thread reads and inflates file i + 1 while the caller works on
    file i -- at most one case ahead; what the thread met is re-raised by `get`.  Headers are read and buffers grown in the
    caller's thread; the thread does file I/O and zlib only (both release the interpreter lock)."""

    def __init__(self, files, device, ahead=True):
        import concurrent.futures
        self.files, self.pin = list(files), torch.device(device).type == "cuda"
        self.bufs, self.uploaded = [None, None], [None, None]
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="volume-reader") if ahead else None
        self.jobs = {}

    def _start(self, i):
        plan = infer_plan(self.files[i])
        slot = i & 1
        if self.uploaded[slot] is not None:                # the upload that last used this buffer has left it
            self.uploaded[slot].synchronize()
            self.uploaded[slot] = None
        if self.bufs[slot] is None or self.bufs[slot].numel() < plan["nbytes"]:
            self.bufs[slot] = torch.empty(plan["nbytes"], dtype=torch.uint8, pin_memory=self.pin)
        view = self.bufs[slot].numpy()[:plan["nbytes"]]
        job = self.pool.submit(read_voxel_block, self.files[i], plan["header"], view) if self.pool is not None else None
        self.jobs[i] = (plan, job, view)

    def prefetch(self, i):
        """Start on file i (no-op past the end, when it is started already, or without the thread)."""
        if self.pool is not None and i < len(self.files) and i not in self.jobs:
            self._start(i)

    def get(self, i):
        """(plan, block): file i's infer_plan and its voxel block, a uint8 host tensor in the staging buffer."""
        if i not in self.jobs:
            self._start(i)
        plan, job, view = self.jobs.pop(i)
        if job is not None:
            job.result()                                   # re-raises the thread's exception, which names the file
        else:
            read_voxel_block(self.files[i], plan["header"], view)
        return plan, self.bufs[i & 1][:plan["nbytes"]]

    def sent(self, i):
        """The caller has queued the upload of file i's block on the current stream."""
        if self.pin:
            self.uploaded[i & 1] = torch.cuda.Event()
            self.uploaded[i & 1].record()

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None


class CaseStore(object):
    """One ingested volume as the windows' kernels see a store (the duck type of lits.SliceStore): `im` the int16-typed storage
    of the uint16 pixels [d, h, w], `lb` zeros of the same shape, the case at offset 0."""

    def __init__(self, im, lb, device):
        self.im, self.lb, self.offset, self.device = im, lb, {0: 0}, device


def input_fn_infer(mode, params):
    """`liver_3d --mode infer`: per input volume (infer_files) the header is read, the voxel block goes
    through VolumeReader into staging memory, is uploaded as it lies in the file and `unetk_nii_ingest` turns it into the
    store's slices on the device -- a CaseStore per case, slices of any one size.  Then exactly what `_eval_cases` yields: the
    case's window tables (here with dict(store=...) beside them, there is no fold-wide store) and the end-of-case item, which
    also carries `header` and `special` for the saver.  --eval_overlap, --eval_mirror, --eval_window_weight and --eval_box_from
    (the box of DIR/predict-<case>.nii.gz) apply unchanged; --eval_in_patches is implied.
    params["infer_read_ahead"] = False reads every file in the caller's thread (measurements)."""
    args = params["args"]
    if mode != "infer" or getattr(args, "mode", "infer") != "infer":
        raise ValueError("lits3d.input_fn_infer serves --mode infer, got {} / --mode {}".format(mode, getattr(args, "mode", None)))
    check_args(args)
    files = infer_files(args, params)
    files = files[int(getattr(args, "eval_skip_num", 0) or 0):]
    if int(getattr(args, "eval_num", -1)) > 0:
        files = files[:int(args.eval_num)]
    return _infer_cases(args, params, files)


def _infer_cases(args, params, files):
    device = params.get("device") or torch.device("cuda", torch.cuda.current_device())
    bs = distribution_utils.per_device_batch_size(args.batch_size, args.num_gpus)
    shape = (int(args.im_depth), int(args.im_height), int(args.im_width))
    variants = mirror_variants(args)
    box_from = getattr(args, "eval_box_from", None)
    mm = z_spacing(args)
    reader = VolumeReader(files, device, ahead=bool(params.get("infer_read_ahead", True)))
    zeros = None                                           # the labels of every case: zeroed once, grown to the largest case
    try:
        for i in range(len(files)):
            plan, block = reader.get(i)
            dev_block = torch.empty(block.numel(), dtype=torch.uint8, device=device)
            dev_block.copy_(block, non_blocking=True)
            reader.sent(i)
            reader.prefetch(i + 1)
            header = plan["header"]
            im = ops.nii_ingest(dev_block, plan["dtype"], plan["file_shape"], plan["trans_bk"], plan["flips"], header.scl_slope,
                                header.scl_inter)
            del dev_block
            depth, src_h, src_w = plan["shape"]
            if zeros is None or zeros.numel() < im.numel():
                zeros = torch.zeros(im.numel(), dtype=torch.uint8, device=device)
            store = CaseStore(im, zeros[:im.numel()].view(im.shape), device)
            case = {"PID": 0, "size": [depth, src_h, src_w]}                   # the one case of its store, at offset 0
            end = dict(case=plan["case"], base=0, depth=depth, store=store, header=header, special=plan["special"])
            box = None
            if box_from is not None:
                box = end["box"] = prediction_box(box_from, plan["case"], depth, (src_h, src_w),
                                                  getattr(args, "eval_box_margin", DEFAULT_BOX_MARGIN), special=plan["special"])
            cd = None
            if mm is not None:                             # --z_spacing: the pixdim of the file axis that became the store's z
                cd = crop_depth(shape[0], mm, infer_spacing(files[i], plan))
                check_crop_limit([cd], (src_h, src_w), [plan["case"]])
            for tab in eval_tables(case, store, shape, float(getattr(args, "eval_overlap", 0.5)), variants, bs, box, cd=cd):
                yield tab, ({"store": store, "zcrop": cd} if cd is not None else {"store": store})
            yield None, end
    finally:
        reader.close()
