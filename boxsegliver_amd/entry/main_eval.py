"""Score the click-guided nets (UNetInter, SmallUNet, InterUNet, LGNet) by simulated corrective clicks -- the drop-in for the
reference's entry/main_eval.py, on LiTS:

    python -m boxsegliver_amd.entry.main_eval --mode eval --tag NAME --model UNetInter --classes Tumor --use_spatial ...

There is no sub-command.  The parser is the reference's (:43-70): config, core.models, loss_metrics, the `liver_inter` flag
group and the "Evaluation Arguments" group with its names and defaults, plus --lits_root and --seed.

Every slice of a case that holds the object is one SESSION (:322-363).  --batch_size sessions run in lockstep; the slots of
finished sessions are refilled from the next slices of the same case.  One ROUND is one launch sequence for the whole batch:
  unetk_inter_click      the prediction of the last forward at source resolution into the case's volume, its counts against
                         the label, and the next click at the centre of the largest error region (inter_simulation_test)
  ONE host read          the int32 [batch, 16] table: the float64 Dice, the stop decisions and the slot refill happen here
  unetk_click_guide_list the guide from all clicks so far (update_guide's running max / min); under --geodesic_guide
                         unetk_click_geodesic on the half-resolution centre channel, computed once per fresh table (:205-220)
  the net                with mirror averaging (run_TTA), arg-max
Per session the order is the reference's (:335-358): click -- stop if it repeats the previous one -- guide, forward -- Dice --
stop if Dice > --inter_thresh or fg + bg clicks >= --max_iter.  The Dice of a forward is read together with the next click,
so a session that stops by its Dice has had one more click computed than it uses; that click is not counted.

Deviations: the images are z-scored at source resolution and resized with align_corners as in training
(unetk_lits_inter_batch; the reference resizes with cv2 first); the nearest resize of the prediction is floor(y * H / src_h);
where the reference asks for a skeleton, the click is the error region's pixel deepest inside it; an empty error mask ends the
session (the reference would raise); --guide_channel 1 with the Euclidean guide feeds fg - bg (the reference feeds zeros)."""
import argparse
import logging
import sys
from pathlib import Path

import numpy as np

from .. import config, loss_metrics
from ..NetworksV2.base import ModeKeys
from ..core import models

log = logging.getLogger("boxsegliver_amd")

LEGACY_FIRST_WORDS = ("nf_inter", "liver_inter")
_FLIPS = ((False, False), (False, True), (True, False), (True, True))   # mirror id -> (flip H, flip W)


def build_parser():
    from ..data import lits_inter
    parser = argparse.ArgumentParser(prog="boxsegliver_amd.entry.main_eval")
    config.add_arguments(parser)
    models.add_arguments(parser)
    loss_metrics.add_arguments(parser)
    lits_inter.add_arguments(parser)
    group = parser.add_argument_group(title="Evaluation Arguments")          # main_eval.py:50-64, verbatim
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
    """main_eval.py:43-70.  Six of the reference's shipped scripts (scripts/102_gnet_v2.sh ...) still pass the pipeline's name
    as a first word, which its parser has no argument for; that word is dropped here so their flag lists parse."""
    parser = build_parser()
    argv = list(argv)
    if argv and argv[0] in LEGACY_FIRST_WORDS:
        argv = argv[1:]
    args = parser.parse_args(argv)
    config.check_args(args, parser)
    config.fill_default_args(args)
    return args


def check_args(args):
    """Refuses what is not built, naming the flag, before anything is loaded; returns the object label."""
    from .. import _abi
    from ..data import lits_inter
    lits_inter.refuse_unbuilt_flags(args)
    if getattr(args, "test", False):
        raise NotImplementedError("--test is not built: it scores the reference's private NF test set")
    if getattr(args, "save_predict", False):
        raise NotImplementedError("--save_predict is not built for the interactive evaluator")
    if getattr(args, "infer_set", "eval") not in ("eval", "train"):
        raise ValueError("--infer_set must be eval or train, got {}".format(args.infer_set))
    if getattr(args, "use_spatial", False) and not 0 <= int(args.max_iter) <= _abi.INTER_MAX_CLICKS:
        raise ValueError("--max_iter must lie in [0, {}] (the click lists live on the device), got {}".format(
            _abi.INTER_MAX_CLICKS, args.max_iter))
    if int(args.im_height) <= 0 or int(args.im_width) <= 0:
        raise ValueError("--im_height and --im_width must be given: the nets are evaluated at their training resolution")
    return lits_inter.check_values(args)


def mirror_plan(args):
    """run_TTA (main_eval.py:262-281): the mirror ids forwarded, the plain one first -- left/right if random_flip & 1, up/down
    if random_flip & 2, both if random_flip & 3 (so --random_flip 1 also runs the double flip).  The probabilities are flipped
    back, summed and divided by len(plan)."""
    plan = [0]
    rf = int(getattr(args, "random_flip", 0) or 0)
    if getattr(args, "eval_mirror", False):
        if rf & 1 > 0:
            plan.append(1)
        if rf & 2 > 0:
            plan.append(2)
        if rf & 3 > 0:
            plan.append(3)
    return plan


def dice(n_pred, n_ref, n_inter):
    """compute_dice (main_eval.py:225-228) from the integer counts, in float64."""
    return (2 * int(n_inter) + 1e-8) / (int(n_pred) + int(n_ref) + 1e-8)


# ------------------------------------------------------------------------------------------------- the session loop
def run_case(lb, slices, predict, pred_hw, batch, max_iter, inter_thresh, obj_label, vol, vol_base, trace=None, case=None,
             trace_preds=False):
    """The interactive sessions of one case.  lb: the store's labels; slices: store indices of the case's object slices;
    predict(pts, cnt, slot_slices, fresh) -> uint8 [batch, H, W] device prediction of every slot (slot_slices: store index or
    -1; fresh: the slots whose session has just begun); vol uint8 [depth, src_h, src_w]: the case's prediction volume, whose
    slice 0 is store slice vol_base.  Returns [fg clicks, bg clicks] summed over the sessions.  One device-to-host read per
    round.  trace: a list that gets one (case, slice, click, kind, fallback, counts, stop reason) per session and round --
    counts = (n_pred, n_ref, n_inter) of the prediction the round began with, click = None where the round placed none, stop
    reason None or "repeat" / "dice" / "max_iter" / "empty"; with trace_preds the record ends with that prediction (host)."""
    import torch

    from .. import _abi, ops
    from ..data import lits
    batch, k = int(batch), max(int(max_iter), 1)
    dev = lb.device
    pts = torch.full((batch, 2, k, 2), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros((batch, 2), dtype=torch.int32, device=dev)
    pred = torch.zeros((batch, int(pred_hw[0]), int(pred_hw[1])), dtype=torch.uint8, device=dev)
    table = torch.empty((batch, _abi.INTER_TAB_COLS), dtype=torch.int32, device=dev)
    ws = ops.inter_click_ws(ops.inter_click_desc(lb, batch, pred_hw, k, obj_label, lits.LB_SCALE, vol_base, vol.shape[0]), dev)
    pending = [int(s) for s in slices]
    slots = [None] * batch
    inters = [0, 0]
    while True:
        fresh = []
        for j in range(batch):
            if slots[j] is None and pending:
                slots[j] = dict(slice=pending.pop(0), prev=(-1, -1), n=[0, 0], round=0)
                fresh.append(j)
        if all(s is None for s in slots):
            return inters
        if fresh:
            idx = torch.tensor(fresh, dtype=torch.int64, device=dev)
            pred.index_fill_(0, idx, 0)                               # round 0: the prediction is all zeros
            cnt.index_fill_(0, idx, 0)
            pts.index_fill_(0, idx, -1)
        rows = np.zeros((batch, _abi.INTER_ROW_COLS), dtype=np.int32)
        for j, s in enumerate(slots):
            rows[j] = (s["slice"], 1) + tuple(s["prev"]) if s is not None else (0, 0, -1, -1)
        rows_d, = lits.upload_pinned([rows], dev)
        ops.inter_click(lb, rows_d, pred, pts, cnt, obj_label, lits.LB_SCALE, vol, vol_base, table=table, ws=ws)
        tab = table.cpu().numpy()                                     # the round's one host read
        for j, s in enumerate(slots):
            if s is None:
                continue
            row = tab[j]
            if row[15] != 1:
                raise RuntimeError("interactive evaluation: slice {} lies outside the store or its case's volume".format(s["slice"]))
            counts, stop, click = tuple(int(v) for v in row[:3]), None, None
            if s["round"] > 0:                                        # :350-358: the forward of the round before
                if dice(*counts) > inter_thresh:
                    stop = "dice"
                elif s["n"][0] + s["n"][1] >= max_iter:
                    stop = "max_iter"
            if stop is None:
                if row[13]:
                    stop = "empty"                                    # nothing to correct (the reference would raise)
                else:
                    click = (int(row[8]), int(row[9]))
                    s["n"][int(row[10])] += 1                         # :221: counted before the repeat test
                    if row[12]:
                        stop = "repeat"                               # :337-341
                    s["prev"] = click
            if trace is not None:
                rec = (case, s["slice"] - vol_base, click, int(row[10]) if click else -1, bool(row[11]) if click else False,
                       counts, stop)
                trace.append(rec + (pred[j].cpu().numpy(),) if trace_preds else rec)
            if stop is not None:
                inters[0] += s["n"][0]
                inters[1] += s["n"][1]
                slots[j] = None
            else:
                s["round"] += 1
        if any(s is not None for s in slots):
            pred = predict(pts, cnt, [s["slice"] if s is not None else -1 for s in slots], fresh)


def run_case_plain(lb, slices, predict, pred_hw, batch, obj_label, vol, vol_base):
    """Without --use_spatial (:359-362): one forward per object slice, no clicks; the click step only resizes the prediction
    into the volume."""
    import torch

    from .. import _abi, ops
    from ..data import lits
    dev = lb.device
    pts = torch.empty((batch, 2, 1, 2), dtype=torch.int32, device=dev)
    cnt = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    slices = [int(s) for s in slices]
    for b0 in range(0, len(slices), batch):
        part = slices[b0:b0 + batch]
        slot_slices = part + [-1] * (batch - len(part))
        pred = predict(None, None, slot_slices, list(range(len(part))))
        rows = np.array([(s, 1, -1, -1) if s >= 0 else (0, 0, -1, -1) for s in slot_slices], dtype=np.int32).reshape(batch, _abi.INTER_ROW_COLS)
        rows_d, = lits.upload_pinned([rows], dev)
        cnt.zero_()
        ops.inter_click(lb, rows_d, pred, pts, cnt, obj_label, lits.LB_SCALE, vol, vol_base)


# ------------------------------------------------------------------------------------------------- the net
class NetPredictor(object):
    """predict() of run_case for a real net: the whole slice through unetk_lits_inter_batch (training = 0, no flips, a crop
    box equal to the slice), the guide from the click lists, the forward under mirror_plan, arg-max (lowest index on ties)."""

    def __init__(self, model, model_args, model_kwargs, store, args, obj_label):
        import torch
        self.model, self.model_args = model, tuple(model_args)
        self.kwargs = dict(model_kwargs, ret_prob=True, ret_pred=False)           # build_graph :253-254
        self.store, self.args, self.obj_label = store, args, obj_label
        self.shape = (int(args.im_channel), int(args.im_height), int(args.im_width))
        self.spatial = bool(getattr(args, "use_spatial", False))
        self.stddev = float(getattr(args, "stddev", 3.)) if getattr(args, "local_enhance", False) else None
        self.channels = int(getattr(args, "guide_channel", 2))
        self.geodesic = self.spatial and bool(getattr(args, "geodesic_guide", False))
        self.plan = mirror_plan(args)
        self.status = torch.zeros(1, dtype=torch.int32, device=store.device)
        self.case = None                                                          # (base, depth) of the case being scored
        self.tab = self.images = self.base = None

    def forward(self, feats):
        self.model(feats, ModeKeys.EVAL, *self.model_args, **self.kwargs)
        return self.model.probability

    def probability(self, feats):
        """run_TTA :262-279."""
        from .. import ops
        prob = self.forward(feats)
        if len(self.plan) == 1:
            return prob
        acc = ops.flip_axpy(prob, None, False, False, 1.0)
        for m in self.plan[1:]:
            fh, fw = _FLIPS[m]
            flipped = {key: ops.flip_axpy(v, None, fh, fw) for key, v in feats.items()}
            ops.flip_axpy(self.forward(flipped), acc, fh, fw, 1.0, accumulate=True)
        return ops.flip_axpy(acc, None, False, False, 1.0 / len(self.plan))

    def __call__(self, pts, cnt, slot_slices, fresh):
        import torch

        from .. import _abi, ops
        from ..data import lits, lits3d
        base, depth = self.case
        src_h, src_w = (int(v) for v in self.store.im.shape[1:])
        if fresh or self.tab is None:
            tab = np.zeros((len(slot_slices), _abi.LITS3D_TAB_COLS), dtype=np.int32)
            tab[:, lits3d.COL_BASE], tab[:, lits3d.COL_DEPTH] = base, depth
            tab[:, lits3d.COL_CZ] = [s - base if s >= 0 else 0 for s in slot_slices]
            tab[:, lits3d.COL_CY], tab[:, lits3d.COL_CX] = src_h // 2, src_w // 2
            tab[:, lits3d.COL_CH], tab[:, lits3d.COL_CW] = src_h, src_w
            tab[:, lits3d.COL_GAMMA] = np.array([1.0], dtype=np.float32).view(np.int32)[0]
            self.tab, = lits.upload_pinned([tab], self.store.device)
            self.images, _ = ops.lits_inter_batch(self.store.im, self.store.lb, self.tab, self.shape, False, self.status,
                                                  self.obj_label, 0.0, 0, lits.IM_SCALE, lits.LB_SCALE)
            if self.geodesic:
                self.base = ops.lits_inter_center(self.store.im, self.tab, self.shape, self.status, lits.IM_SCALE)
        feats = {"images": self.images}
        if self.geodesic:
            feats["sp_guide"] = ops.click_geodesic(self.tab, self.base, pts, cnt, self.shape[1:], self.channels, status=self.status,
                                                   src_hw=(src_h, src_w))
        elif self.spatial:
            feats["sp_guide"] = ops.click_guide_list(self.tab, pts, cnt, self.shape[1:], (src_h, src_w), self.channels, self.stddev)
        prob = self.probability(feats)
        amax, _ = ops.head_predict(prob.contiguous(), prob.shape[-1], want_preds=False)
        return amax.view(prob.shape[0], prob.shape[1], prob.shape[2])


# ------------------------------------------------------------------------------------------------- the run
def _setup_logging(args):
    log_dir = Path(args.model_dir) / "logs"
    log_dir.mkdir(parents=True, exist_ok=True)
    handler = logging.FileHandler(str(log_dir / (args.out_file or "{}_{}".format(args.mode, args.tag))))
    handler.setFormatter(logging.Formatter("%(asctime)s %(levelname)s %(message)s"))
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    return handler


def run(args, dataset_params=None, trace=None, trace_preds=False, restore=True, volumes=None):
    """main_eval.py:284-392 on LiTS.  Returns the results dict: <cls>/<metric> (means over the cases), G_Dice (from the summed
    tp / fp / fn), inters_fg, inters_bg (clicks per case).  trace: see run_case.  restore=False scores the freshly initialised
    variables (tests).  volumes: a dict that gets {pid: the case's prediction volume, uint8 device tensor}."""
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
        net = NetPredictor(model, mparams.get("model_args", ()), mparams.get("model_kwargs", {}), store, args, obj_label)
        spatial = bool(getattr(args, "use_spatial", False))
        batch = int(args.batch_size)
        if model.params is None:                                   # a forward on zeros creates the variables
            feats = {"images": torch.zeros((batch,) + net.shape[1:] + net.shape[:1], dtype=torch.float32, device=device)}
            if spatial:
                feats["sp_guide"] = torch.zeros((batch,) + net.shape[1:] + (net.channels,), dtype=torch.float32, device=device)
            net.forward(feats)
        if ckpt:
            estimator_lib.restore_variables(ckpt, model, None)
        cls = list(args.classes)[-1]
        metrics = list(getattr(args, "metrics_eval", ["Dice"]))
        accu, total, tp, fp, fn = {}, [0, 0], 0, 0, 0
        for case in cases:
            pid, depth = int(case["PID"]), int(case["size"][0])
            base = store.offset[pid]
            net.case, net.tab = (base, depth), None
            vol = torch.zeros((depth,) + tuple(store.lb.shape[1:]), dtype=torch.uint8, device=device)
            slices = [base + z for z in range(depth) if has_obj[base + z]]
            if spatial:
                inters = run_case(store.lb, slices, net, net.shape[1:], batch, int(args.max_iter), float(args.inter_thresh),
                                  obj_label, vol, base, trace, pid, trace_preds)
            else:
                inters = [0, 0]
                run_case_plain(store.lb, slices, net, net.shape[1:], batch, obj_label, vol, base)
            lits_status = int(net.status.item())
            if lits_status:
                raise RuntimeError("interactive evaluation: the image kernels' status word is {}".format(lits_status))
            label = (store.lb[base:base + depth] >= thr).to(torch.uint8) if thr <= 255 else torch.zeros_like(vol)
            conf = ops.mask_counts(vol, label)
            case_metrics = loss_metrics.metric_3d_device(vol, label, required=metrics)
            for key, value in case_metrics.items():
                accu.setdefault("{}/{}".format(cls, key), []).append(value)
            tp, fp, fn = tp + conf["tp"], fp + conf["fp"], fn + conf["fn"]
            total[0] += inters[0]
            total[1] += inters[1]
            if volumes is not None:
                volumes[pid] = vol
            case_metrics = dict(case_metrics, fn=conf["fn"], fp=conf["fp"], tp=conf["tp"])
            log.info("Evaluate-%s%s%s", pid, "".join(" {}: {:.3f}".format(key, v) for key, v in case_metrics.items()),
                     " (Num inters: {})".format(inters) if spatial else "")
        results = {key: float(np.mean(v)) for key, v in accu.items()}
        results["G_Dice"] = 2 * tp / (2 * tp + fn + fp) if 2 * tp + fn + fp else 0.0
        n = len(cases)
        log.info("---Infer %d cases%s%s", n, "".join(" - {}: {:.3f}".format(key, v) for key, v in results.items()),
                 " (Average inters: {:.1f}/{:.1f})".format(total[0] / n, total[1] / n) if spatial else "")
        results["inters_fg"], results["inters_bg"] = total[0] / n, total[1] / n
        return results
    finally:
        log.removeHandler(handler)
        handler.close()


def main(argv=None):
    run(get_arguments(list(sys.argv[1:] if argv is None else argv)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
