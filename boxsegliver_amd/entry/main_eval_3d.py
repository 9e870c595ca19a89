"""Score a click-guided UNet3D by simulated 3-D corrective clicks -- the drop-in for the reference's entry/main_eval_3d.py,
on LiTS:

    python -m boxsegliver_amd.entry.main_eval_3d --mode eval --tag NAME --model UNet3D --classes Tumor --im_depth 10 \\
        --im_height 256 --im_width 256 --use_spatial [--local_enhance --stddev 1 3 3] ...

There is no sub-command.  The parser is the reference's (:44-71): config, core.models, loss_metrics, the `liver_3d` flag group
(with --eval_overlap, --eval_window_weight/_sigma, --eval_box_from/_margin) and the "Evaluation Arguments" group with its names
and defaults, plus --lits_root and --seed.  The flags of `nf_3d` that `liver_3d` lacks live in a group of this module only, so
that every `main_eval_3d` line of the reference's shipped scripts parses; those that are not built are refused by name.

A case is one SESSION (:312-385); cases without an object voxel are skipped.  One ROUND is one launch sequence:
  unetk_inter_click3d       the counts of the case's resident prediction volume against the label, the next click at the centre
                            of the largest error region (inter_simulation_test) and its append to the case's click lists
  ONE host read             the int32 [20] table row: the float64 Dice and the stop decision happen here
  per window table          unetk_click_guide3d_list (the guide of those windows from ALL clicks so far: update_guide's running
                            max / min), unetk_lits_patch3d, the net, unetk_eval3d_accumulate[_w]  (evaluator_liver.CaseWindows3D,
                            the loop EvaluateVolume.run_3d runs)
  finish                    the class volume uint8 [depth, src_h, src_w], resident
Per session the order is the reference's (:341-384): click -- stop if it repeats the previous one -- guide, forward -- Dice --
stop if Dice > --inter_thresh or fg + bg clicks >= --max_iter.  The Dice of a forward is read together with the next click, so
a session that stops by its Dice or by --max_iter has had one more click computed than it uses; that click is not counted.
Without --use_spatial: one pass and no clicks (:386-389).

With --slice_prior boundary | binary (the reference's --use_cascade [--cascade_binary] without --use_2d,
:348-369) the windows' images carry a second channel: the object on the slice of the session's FIRST foreground click.  Its
field is built ONCE per session (the reference's `pred_2d_added`), by unetk_slice_prior_field over the whole slice of pts[0][0]
read on the device, before the first forward; every window table of every later round renders it through
unetk_slice_prior_render's shared form, however many clicks follow.  Round 0 starts from an empty prediction, so every error
voxel is an object voxel and its click is a foreground click: the field always has its slice.  Were there none, the channel
would be zeros (the reference's `len(pos_col[0]) == 0` branch).  --use_cascade and --cascade_binary themselves stay refused as
before; the variant that feeds a 2-D net's prediction (--use_2d, infer_2d.py) needs a second checkpoint and is not built.

Deviations: the net runs in windows of its training depth in place of one forward over the whole case
(--im_depth <= 0 is refused); the guide is rendered as in training, at crop resolution and resized with align_corners (the
reference zooms a source-resolution guide with ndi.zoom); the images go through unetk_lits_patch3d(training = 0); where the
reference asks for a skeleton, the click is the error region's voxel deepest inside it; an empty error mask ends the session
(the reference would raise); filter_tiny_nf is not applied to the labels; --guide_channel 1 feeds fg - bg."""
import argparse
import logging
import sys

import numpy as np

from .. import config, loss_metrics
from ..NetworksV2.base import ModeKeys
from ..core import models
from ..data import flagsets
from .main_eval import _setup_logging, dice

log = logging.getLogger("boxsegliver_amd")

NF_3D_ONLY = [name for name in flagsets.PIPELINES["nf_3d"][0] if name not in flagsets.PIPELINES["liver_3d"][0]]
NOT_BUILT = (("use_cascade", "--use_cascade", "the cascade feeds a 2-D net's prediction as a second image channel; the prior "
                                             "built from the label is --slice_prior boundary"),
             ("cascade_binary", "--cascade_binary", "the cascade feeds a 2-D net's prediction as a second image channel; the "
                                                    "prior built from the label is --slice_prior binary"),
             ("downsampling", "--downsampling", "the resident store holds the slices at full resolution"),
             ("test", "--test", "it scores the reference's private NF test set"),
             ("save_predict", "--save_predict", "the interactive evaluator writes no volumes"))


def build_parser():
    from ..data import lits3d
    parser = argparse.ArgumentParser(prog="boxsegliver_amd.entry.main_eval_3d")
    config.add_arguments(parser)
    models.add_arguments(parser)
    loss_metrics.add_arguments(parser)
    lits3d.add_arguments(parser, z_spacing=False)                            # the sessions need --use_spatial, which the flag refuses
    group = parser.add_argument_group(title="Input Pipeline Arguments (nf_3d only)")
    for name in NF_3D_ONLY:                                                  # input_pipeline_3d.py:53-80, names / defaults verbatim
        kw = dict(flagsets.FLAGS[name])
        group.add_argument(*kw.pop("flags", (name,)), **kw)
    group = parser.add_argument_group(title="Evaluation Arguments")          # main_eval_3d.py:51-65, verbatim
    group.add_argument("--eval_final", action="store_true", required=False,
                       help="Evaluate with final checkpoint. If not set, then evaluate with best checkpoint(default).")
    group.add_argument("--ckpt_path", type=str, required=False,
                       help="Given a specified checkpoint for evaluation. (default best checkpoint)")
    group.add_argument("--save_path", type=str, default="prediction")
    group.add_argument("--inter_thresh", type=float, default=0.9, help="Threshold of the segmentation goal")
    group.add_argument("--max_iter", type=int, default=20, help="Maximum iters for each image in interaction")
    group.add_argument("--infer_set", type=str, default="eval", help="Choice from [train, eval]")
    group.add_argument("--save_subdir", type=str, default="prediction")
    group.add_argument("--test", action="store_true")
    return parser


def get_arguments(argv):
    """main_eval_3d.py:44-71."""
    parser = build_parser()
    args = parser.parse_args(list(argv))
    config.check_args(args, parser)
    config.fill_default_args(args)
    return args


def object_label(classes):
    """--classes -> the stored label from which a voxel is the object: the forced class of `liver_3d --use_spatial` (the
    tumour where it is a class, else the liver).  The net's object class is its last one."""
    classes = tuple(classes)
    if classes not in (("Liver",), ("Tumor",), ("Liver", "Tumor")):
        raise ValueError("the LiTS labels serve --classes Liver, Tumor or Liver Tumor, got {}".format(" ".join(classes)))
    return 2 if "Tumor" in classes else 1


def check_args(args):
    """Refuses what is not built, naming the flag, before anything is loaded; returns the object label."""
    from .. import _abi
    from ..data import lits3d
    for attr, flag, why in NOT_BUILT:
        if getattr(args, attr, False):
            raise NotImplementedError("{} is not built: {}".format(flag, why))
    if int(args.im_depth) <= 0:
        raise ValueError("--im_depth must be > 0: the reference's single forward over a case's whole depth is not built "
                         "(DESIGN.md 7.3.4); the net is run in windows of its training depth, got {}".format(args.im_depth))
    if int(args.im_height) <= 0 or int(args.im_width) <= 0:
        raise ValueError("--im_height and --im_width must be given: the net is evaluated at its training resolution")
    if not 0 <= int(args.max_iter) <= _abi.INTER_MAX_CLICKS:
        raise ValueError("--max_iter must lie in [0, {}] (the click lists live on the device), got {}".format(
            _abi.INTER_MAX_CLICKS, args.max_iter))
    if getattr(args, "infer_set", "eval") not in ("eval", "train"):
        raise ValueError("--infer_set must be eval or train, got {}".format(args.infer_set))
    lits3d.check_values(args)
    return object_label(args.classes)


# ------------------------------------------------------------------------------------------------- the session loop
def run_session(lb, base, depth, predict, max_iter, inter_thresh, obj_label, trace=None, case=None, trace_preds=False):
    """The interactive session of one case.  lb: the store's labels; the case is store slices [base, base + depth);
    predict(pts, cnt) -> uint8 [depth, src_h, src_w] device volume, non-zero = object, from the click lists pts int32
    [2, K, 3] / cnt int32 [2] in case coordinates.  Returns ([fg clicks, bg clicks], the last prediction or None).  One
    device-to-host read per round.  trace: a list that gets one (case, click, kind, fallback, counts, stop reason) per round --
    counts = (n_pred, n_ref, n_inter) of the prediction the round began with, click = None where the round placed none,
    stop reason None or "repeat" / "dice" / "max_iter" / "empty"; with trace_preds the record ends with that prediction (host,
    None in round 0)."""
    import torch

    from .. import _abi, ops
    from ..data import lits
    k = max(int(max_iter), 1)
    dev = lb.device
    pts = torch.full((2, k, 3), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    table = torch.empty(_abi.INTER3D_TAB_COLS, dtype=torch.int32, device=dev)
    ws = ops.inter_click3d_ws(ops.inter_click3d_desc(lb, base, depth, k, obj_label, lits.LB_SCALE), dev)
    pred, prev, n, rounds = None, None, [0, 0], 0                     # round 0: the prediction is all zeros
    while True:
        ops.inter_click3d(lb, base, depth, pred, prev, pts, cnt, obj_label, lits.LB_SCALE, table=table, ws=ws)
        row = table.cpu().numpy()                                     # the round's one host read
        if row[17] != 1:
            raise RuntimeError("interactive evaluation: case {} lies outside the store".format(case))
        counts, stop, click = tuple(int(v) for v in row[:3]), None, None
        if rounds > 0:                                                # :376-384: the forward of the round before
            if dice(*counts) > inter_thresh:
                stop = "dice"
            elif n[0] + n[1] >= max_iter:
                stop = "max_iter"
        if stop is None:
            if row[15]:
                stop = "empty"                                        # nothing to correct (the reference would raise)
            else:
                click = tuple(int(v) for v in row[9:12])
                n[int(row[12])] += 1                                  # :206: counted before the repeat test
                if row[14]:
                    stop = "repeat"                                   # :343-347
                prev = click
        if trace is not None:
            rec = (case, click, int(row[12]) if click else -1, bool(row[13]) if click else False, counts, stop)
            trace.append(rec + (None if pred is None else pred.cpu().numpy(),) if trace_preds else rec)
        if stop is not None:
            return n, pred
        rounds += 1
        pred = predict(pts, cnt)


# ------------------------------------------------------------------------------------------------- the net
class NetPredictor(object):
    """predict() of run_session for UNet3D: the case's window tables (lits3d.eval_tables, mirror variants as rows), per table
    the guide of its rows from the click lists, through evaluator_liver.CaseWindows3D."""

    def __init__(self, model, model_args, model_kwargs, store, args):
        from ..data import lits3d
        from ..evaluators.evaluator_liver import CaseWindows3D
        self.model, self.model_args = model, tuple(model_args)
        self.kwargs = dict(model_kwargs, ret_prob=True, ret_pred=False)           # build_graph :237-238
        self.store, self.args = store, args
        self.shape = (int(args.im_depth), int(args.im_height), int(args.im_width))
        self.guide = lits3d.guide_config(args)
        self.prior = lits3d.slice_prior(args)                                     # None | "boundary" | "binary"
        self.obj_label = object_label(args.classes)
        self.field = None                                                         # (field, z0) of the session, built once
        self.n_classes = len(tuple(args.classes))
        self.variants = lits3d.mirror_variants(args)
        self.windows = CaseWindows3D(self.forward, args)
        self.tables = self.box = None                                             # of the case being scored
        self.coverage = None

    def forward(self, feats):
        self.model(feats, ModeKeys.EVAL, *self.model_args, **self.kwargs)
        return self.model.probability

    def begin_case(self, case):
        from ..data import lits3d
        a, store = self.args, self.store
        depth = int(case["size"][0])
        self.box = None
        if getattr(a, "eval_box_from", None) is not None:
            self.box = lits3d.prediction_box(a.eval_box_from, case, depth, store.im.shape[1:],
                                             getattr(a, "eval_box_margin", lits3d.DEFAULT_BOX_MARGIN))
        self.tables = list(lits3d.eval_tables(case, store, self.shape, float(getattr(a, "eval_overlap", 0.5)), self.variants,
                                              int(a.batch_size), self.box))
        self.coverage = None
        self.field = None                                                         # a new session: a new first click

    def classes(self, pts=None, cnt=None):
        """The case's class volume uint8 [depth, src_h, src_w] under the click lists (None: no guide)."""
        from .. import ops
        sp_guide = prior = None
        src_hw = tuple(self.store.im.shape[1:])
        if self.prior is not None:
            from ..data import lits
            if self.field is None:                                                # once per session, from the first click
                (row,) = lits.upload_pinned([self.tables[0][:1]], self.store.device)
                self.field = ops.slice_prior_field(self.store.lb, row, pts, cnt, self.shape, self.obj_label, self.prior,
                                                   whole=True, lab_scale=lits.LB_SCALE)
            field, z0 = self.field

            def prior(dtab, images):
                return ops.slice_prior_render(dtab, images, field, z0, self.shape, src_hw, self.prior, shared=True)
        if self.guide is not None:

            def sp_guide(dtab):
                return ops.click_guide3d_list(dtab, pts, cnt, self.shape, src_hw, self.guide["channels"], self.guide["stddev"])
        for tab in self.tables:
            self.windows.add(self.store, tab, sp_guide=sp_guide, prior=prior)
        volume, self.coverage = self.windows.finish(self.box)
        return volume

    def binary(self, volume):
        """non-zero = the object: the net's last class."""
        return volume if self.n_classes == 1 else (volume >= self.n_classes).to(volume.dtype)

    def check_coverage(self, pid):
        """Read where the case's scoring synchronises anyway."""
        cov = self.coverage
        if cov is not None and ((int(cov.item()) != 0) if cov.dim() == 1 else (int(cov.min().item()) <= 0)):
            raise RuntimeError("the windows do not cover every voxel of case {}".format(pid))


# ------------------------------------------------------------------------------------------------- the run
def run(args, dataset_params=None, trace=None, trace_preds=False, restore=True, volumes=None):
    """main_eval_3d.py:290-420 on LiTS.  Returns the results dict: <cls>/<metric> (means over the cases), G_Dice (from the
    summed tp / fp / fn), inters_fg, inters_bg (clicks per case).  trace: see run_session.  restore=False scores the freshly
    initialised variables (tests).  volumes: a dict that gets {pid: the case's final class volume, uint8 device tensor}."""
    obj_label = check_args(args)                                  # refusals raise before anything is loaded
    import torch

    from .. import ops
    from ..core import estimator as estimator_lib
    from ..data import lits
    from ..utils import tf_checkpoint
    handler = _setup_logging(args)
    try:
        log.debug(args)
        params = dict(dataset_params or {})
        root = params.get("lits_root", args.lits_root)
        device = params.get("device", torch.device("cuda", torch.cuda.current_device()))
        mparams = models.get_model_params(args)
        model = mparams["model"](args)
        ckpt = None
        if restore:
            ckpt = args.ckpt_path or tf_checkpoint.get_checkpoint_state(args.model_dir, None if args.eval_final else args.load_status_file)
            if not ckpt or not tf_checkpoint.checkpoint_exists(ckpt):
                raise FileNotFoundError("Missing checkpoint file in {} with status_file {}".format(
                    args.model_dir, None if args.eval_final else args.load_status_file))
        cases = lits.collect_datasets(root, args.test_fold, "train" if args.infer_set == "train" else "val",
                                      filter_tumor_size=getattr(args, "filter_size", 0))
        if len(cases) == 0:
            raise ValueError("No valid dataset found!")
        store = lits.SliceStore(root, cases, device)
        thr = obj_label * lits.LB_SCALE
        has_obj = (store.lb >= thr).flatten(1).any(dim=1).cpu().numpy() if thr <= 255 else np.zeros(store.lb.shape[0], bool)
        net = NetPredictor(model, mparams.get("model_args", ()), mparams.get("model_kwargs", {}), store, args)
        spatial = net.guide is not None
        if model.params is None:                                   # a forward on zeros creates the variables
            feats = {"images": torch.zeros((1,) + net.shape + (int(args.im_channel),), dtype=torch.float32, device=device)}
            if spatial:
                feats["sp_guide"] = torch.zeros((1,) + net.shape + (net.guide["channels"],), dtype=torch.float32, device=device)
            net.forward(feats)
        if ckpt:
            estimator_lib.restore_variables(ckpt, model, None)
        cls = list(args.classes)[-1]
        metrics = list(getattr(args, "metrics_eval", ["Dice"]))
        accu, total, tp, fp, fn, scored = {}, [0, 0], 0, 0, 0, 0
        for case in cases:
            pid, depth = int(case["PID"]), int(case["size"][0])
            base = store.offset[pid]
            if not has_obj[base:base + depth].any():               # load_dataset :112-113: nf_set holds the cases with an object
                continue
            scored += 1
            net.begin_case(case)
            if spatial:
                state = {}

                def predict(pts, cnt):
                    state["classes"] = net.classes(pts, cnt)
                    return net.binary(state["classes"])
                inters, vol = run_session(store.lb, base, depth, predict, int(args.max_iter), float(args.inter_thresh),
                                          obj_label, trace, pid, trace_preds=trace_preds)
                classes = state.get("classes")
            else:
                inters = [0, 0]
                classes = net.classes()
                vol = net.binary(classes)
            if vol is None:                                        # no forward ran: nothing is predicted
                vol = classes = torch.zeros((depth,) + tuple(store.lb.shape[1:]), dtype=torch.uint8, device=device)
            net.check_coverage(pid)
            label = (store.lb[base:base + depth] >= thr).to(torch.uint8)
            conf = ops.mask_counts(vol, label)
            case_metrics = loss_metrics.metric_3d_device(vol, label, required=metrics)
            for key, value in case_metrics.items():
                accu.setdefault("{}/{}".format(cls, key), []).append(value)
            tp, fp, fn = tp + conf["tp"], fp + conf["fp"], fn + conf["fn"]
            total[0] += inters[0]
            total[1] += inters[1]
            if volumes is not None:
                volumes[pid] = classes
            case_metrics = dict(case_metrics, fn=conf["fn"], fp=conf["fp"], tp=conf["tp"])
            log.info("Evaluate-%s%s%s", pid, "".join(" {}: {:.3f}".format(key, v) for key, v in case_metrics.items()),
                     " (Num inters: {})".format(inters) if spatial else "")
        if scored == 0:
            raise ValueError("No case of the set holds the object (stored label >= {})".format(obj_label))
        results = {key: float(np.mean(v)) for key, v in accu.items()}
        results["G_Dice"] = 2 * tp / (2 * tp + fn + fp) if 2 * tp + fn + fp else 0.0
        log.info("---Infer %d cases%s%s", scored, "".join(" - {}: {:.3f}".format(key, v) for key, v in results.items()),
                 " (Average inters: {:.1f}/{:.1f})".format(total[0] / scored, total[1] / scored) if spatial else "")
        results["inters_fg"], results["inters_bg"] = total[0] / scored, total[1] / scored
        return results
    finally:
        log.removeHandler(handler)
        handler.close()


def main(argv=None):
    run(get_arguments(list(sys.argv[1:] if argv is None else argv)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
