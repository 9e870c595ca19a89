"""Volume evaluator for liver / tumor segmentation -- host-side mirror of the reference's
evaluators/evaluator_liver.py (`EvaluateVolume`: run :704-766, _predict_case :616-678, _postprocess :680-702,
_run_actual :906-996, _compare :1193-1227) on the libunetk HIP kernels.

What runs where (MI355X-first):
  * HOST or DEVICE (volumes_on): the network's input slabs.  volumes_on="host" (the default) takes the reference's host
    generator: window, bilinear resize and the slabs in numpy, one upload per slab (data/lits.py).  volumes_on="device"
    (what entry/main.py asks for; main_g keeps "host") uploads a case's raw int16 crop once and builds every slab there: `unetk_eval_slab`,
    bit-equal to the host pipeline.
  * DEVICE: the forward passes of every slab, the mirror test-time augmentation (flip of the input slab, un-flip and
    `/ mirror_div` accumulation of the class probabilities: `unetk_flip_axpy`; the reference does this with np.flip
    on the host, :648-655), the concatenation of a case's slabs, and the final `np.argmax(volume, -1)` (:663,
    `unetk_head_predict`, lowest index on ties like numpy).
  * HOST or DEVICE (volumes_on): zoom back to the original shape.  "host": one device->host copy per case (uint8 mask)
    and scipy.ndimage.zoom inside _predict_case.  "device": `unetk_zoom_nearest3d` with index tables asked of scipy itself
    (ops.zoom_tables), so scipy's zero samples just outside the input are reproduced; the prediction stays on the device.
  * DEVICE again (metrics_on="device", the default): the case's labels are uploaded once (and, with volumes_on="host", its
    argmax volume again), then class split, merge tumor into liver, largest connected component (_postprocess_device),
    the per-case volume metrics (loss_metrics.metric_3d_device) and the global Dice counts run in csrc/evalvol.hip.
    metrics_on="host" keeps the reference's host path (_postprocess, loss_metrics.metric_3d, ConfusionMatrix).
    --eval_detection adds per-lesion detection of the Tumor class to either path (loss_metrics.tumor_detection_metrics_device:
    `unetk_component_overlaps`, one table read, the matching on the host; or tumor_detection_metrics).
  * DEVICE, then a HOST THREAD (-s/--save_predict, `maybe_save_case` :998-1026; _CaseSaver below): a case that
    is on the device and scored there is post-processed once, composed into the whole volume in NIfTI file order by
    `unetk_nii_compose` and copied once into a pinned buffer on a side stream; utils/volume_writer writes
    `predict-<case>.nii.gz` (header of the case's volume file, or one built from meta.json) behind the next case.  Host
    volumes take the reference's np.pad / write_nii steps in that thread; the bytes are the same.  --mode infer writes the
    files and scores nothing.

The input contract is the reference's eval generator (DataLoader/Liver/input_pipeline_li.py:398-456): a stream of
`(features, None)` slabs -- features["images"] [bs,H,W,C], features["names"], optional features["mirror"] in {0,1,2,3}
-- closed per case by `(None, (segmentation, vol_path, pads, bbox, resize))`.  When --eval_mirror is set and the
pipeline does NOT emit mirrored copies (no "mirror" key), the evaluator mirrors on the device itself, which saves the
host flips and three host->device copies per slab.

With --use_spatial, `run_g` (evaluator_liver.py:768-917) evaluates by guide propagation instead: data/propagate.py holds the
state machine, `_GuidedLoop` the per-slice device work (one forward, unetk_guide_components, one table copy, unetk_guide_render).

UNet3D on LiTS (`liver_3d --eval_in_patches`) is scored by `run_3d`: sliding windows from data/lits3d.input_fn_eval, one forward per
batch, `unetk_eval3d_accumulate` into the case at source resolution, then the same scoring.  With --mode infer
the cases are NIfTI volumes ingested on the device (data/lits3d.input_fn_infer): no labels, no metrics, and the
saved files carry the input's header; --pred_type prob saves `prob-<case>-<Class>.nii.gz` from the accumulator (`unetk_eval3d_prob`).
"""
import json
import logging
import time
from collections import defaultdict
from pathlib import Path

import numpy as np
import scipy.ndimage as ndi
import torch

from .. import loss_metrics as metric_ops
from .. import ops
from ..NetworksV2.base import ModeKeys
from ..utils import array_kits as arr_ops
from ..utils import tf_checkpoint
from .evaluator_base import EvaluateBase

log = logging.getLogger("boxsegliver_amd")

DETECTION_CLASS = "Tumor"            # --eval_detection: the class whose objects are lesions


def add_arguments(parser):
    """evaluators/evaluator_liver.py:36-71 (names / defaults verbatim)."""
    group = parser.add_argument_group(title="Evaluation Arguments")
    group.add_argument("--primary_metric", type=str, required=False,
                       help="Primary metric for evaluation. Typically it has format <class>/<metric>")
    group.add_argument("--secondary_metric", type=str, required=False,
                       help="Secondary metric for evaluation. Typically it has format <class>/<metric>")
    group.add_argument("--eval_final", action="store_true", required=False,
                       help="Evaluate with final checkpoint. If not set, then evaluate with best checkpoint(default).")
    group.add_argument("--ckpt_path", type=str, required=False,
                       help="Given a specified checkpoint for evaluation. (default best checkpoint)")
    group.add_argument("--evaluator", type=str, choices=["Volume"])
    group.add_argument("--eval_num", type=int, default=-1, required=False, help="Number of cases for evaluation")
    group.add_argument("--eval_skip_num", type=int, default=0, required=False,
                       help="Skip some cases for evaluating determined case")
    group.add_argument("--eval_3d", action="store_true", required=False,
                       help="Evaluate in 2D slices or 3D volume when training. Default in 2D slices")
    group.add_argument("--pred_type", type=str, choices=["pred", "prob"], default="pred",
                       help="Generate prediction or probability")
    group.add_argument("--save_path", type=str, default="prediction")
    group.add_argument("--use_global_dice", action="store_true")
    # project extensions (off by default)
    group.add_argument("--eval_detection", action="store_true",
                       help="Also score per-lesion detection of the Tumor class: <Tumor>/DetTP, DetFP, DetPos, Precision, Recall")
    group.add_argument("--detection_thresh", type=float, default=0.5,
                       help="--eval_detection: a reference lesion is found when its Dice coefficient with a predicted object "
                            "(2 overlap / (size + size); the reference code names it iou) reaches this value")


def get_evaluator(evaluator, estimator=None, model_dir=None, params=None, merge_tumor_to_liver=True, largest=True,
                  use_sg_reduce_fp=False, metrics_on="device", volumes_on="host"):
    if evaluator == "Volume":
        return EvaluateVolume(estimator, model_dir=model_dir, params=params, merge_tumor_to_liver=merge_tumor_to_liver,
                              largest=largest, use_sg_reduce_fp=use_sg_reduce_fp, metrics_on=metrics_on,
                              volumes_on=volumes_on)
    raise ValueError("Unsupported evaluator: {}. Must be [Volume, ]".format(evaluator))


def mirror_plan(config):
    """(variants, divisor) of the mirror TTA exactly as the reference emits / averages them:
    variants after the un-mirrored slab are 1 = flip W if random_flip & 1, 2 = flip H if random_flip & 2,
    3 = both if random_flip & 3 (input_pipeline_li.py:440-455 -- so random_flip 1 or 2 yields TWO extra variants);
    divisor 2 for random_flip in {1, 2}, 4 for 3, else 1 (evaluator_liver.py:114-122)."""
    if not getattr(config, "eval_mirror", False):
        return [], 1
    rf = int(getattr(config, "random_flip", 0) or 0)
    variants = []
    if rf & 1 > 0:
        variants.append(1)
    if rf & 2 > 0:
        variants.append(2)
    if rf & 3 > 0:
        variants.append(3)
    div = 2 if rf in (1, 2) else (4 if rf == 3 else 1)
    return variants, div


_FLIPS = {0: (False, False), 1: (False, True), 2: (True, False), 3: (True, True)}   # mirror id -> (flip H, flip W)


class CaseWindows3D(object):
    """The body of the sliding-window evaluation of ONE case by UNet3D, shared by EvaluateVolume.run_3d and the interactive
    evaluator (entry/main_eval_3d.py): per table `add` -- one pinned upload, the windows cut by `unetk_lits_patch3d` as
    `eval_online` cuts them, one forward, `unetk_eval3d_accumulate[_w]` into the case's accumulator at source resolution --
    and at the end of the case `finish`, the class volume.  forward(features) -> probabilities [n, D, H, W, C].  The options
    are `sp_guide`: a function of the device table that returns the guide feature of its rows, and `prior`: a function of the
    device table and its one-channel images that returns the images the net is fed (--slice_prior: the second channel)."""

    def __init__(self, forward, cfg):
        from ..data import lits3d
        self.forward = forward
        self.shape = (int(cfg.im_depth), int(cfg.im_height), int(cfg.im_width))
        self.lab_max = len(tuple(cfg.classes))
        self.gaussian = getattr(cfg, "eval_window_weight", "uniform") == "gaussian"
        self.boxed = getattr(cfg, "eval_box_from", None) is not None
        self.host_tables = lits3d.window_weights(self.shape, getattr(cfg, "eval_window_sigma", 0.125)) if self.gaussian else None
        self.acc = self.cnt = self.tables = self.kept = None

    def add(self, store, tab, sp_guide=None, before_forward=None, prior=None, zcrop=None):
        """zcrop: the crop depth of the table's windows with --z_spacing (one case, so one value): it rides
        beside the table in the same upload as int32 [n], and the _z entries cut the windows and take them back."""
        from ..data import lits, lits3d
        shape = self.shape
        zkw = {}
        if zcrop is None:
            (dtab,) = lits.upload_pinned([tab], store.device)
        else:
            dtab, dz = lits.upload_pinned([tab, np.full(len(tab), int(zcrop), dtype=np.int32)], store.device)
            zkw = dict(zcrop=dz, zcrop_max=int(zcrop))
        images, _ = ops.lits_patch3d(store.im, store.lb, dtab, shape, False, self.lab_max, lits.IM_SCALE, lits.LB_SCALE, **zkw)
        features = {"images": images if prior is None else prior(dtab, images)}
        if sp_guide is not None:
            features["sp_guide"] = sp_guide(dtab)
        if before_forward is not None:
            before_forward(features)
        prob = self.forward(features).contiguous()                      # [n, D, H, W, C]
        base, depth = int(tab[0, lits3d.COL_BASE]), int(tab[0, lits3d.COL_DEPTH])
        src_hw = tuple(store.im.shape[1:])
        if self.acc is None:
            self.acc = torch.zeros((depth,) + src_hw + (prob.shape[-1],), dtype=torch.float32, device=store.device)
            self.cnt = torch.zeros((depth,) + src_hw, dtype=torch.float32 if self.gaussian else torch.int32, device=store.device)
        box = lits3d.table_box(tab, shape, depth, src_hw, cd=zcrop)
        if self.gaussian:
            if self.tables is None:                                     # once per run
                self.tables = lits.upload_pinned(list(self.host_tables), store.device)
            ops.eval3d_accumulate_w(prob, dtab, shape, base, depth, box, self.tables, self.acc, self.cnt, store.im, host_tab=tab,
                                    **zkw)
        else:
            ops.eval3d_accumulate(prob, dtab, shape, base, depth, box, self.acc, self.cnt, store.im, host_tab=tab, **zkw)

    def labels(self, store, base, depth):
        from ..data import lits
        lb = store.lb[base:base + depth]
        return torch.clamp(torch.div(lb, lits.LB_SCALE, rounding_mode="floor"), max=self.lab_max).to(torch.uint8)

    def finish(self, box=None, keep=False):
        """(class volume uint8 [depth, src_h, src_w], coverage): the coverage volume of the plain path, or the word [1] that
        `unetk_eval3d_finish` counted the box's voxels without cover into.  The case's accumulator is dropped, or with keep
        (--pred_type prob) handed back in `self.kept` = (acc, weight) for `unetk_eval3d_prob`."""
        acc, cnt = self.acc, self.cnt
        self.acc = self.cnt = None
        self.kept = (acc, cnt) if keep else None
        if self.gaussian or self.boxed:
            uncovered = torch.zeros(1, dtype=torch.int32, device=acc.device)
            whole = (0, acc.shape[0], 0, acc.shape[1], 0, acc.shape[2])
            return ops.eval3d_finish(acc, cnt, box if box is not None else whole, uncovered), uncovered
        amax, _ = ops.head_predict(acc.view(-1, acc.shape[-1]), acc.shape[-1], want_preds=False)
        return amax.view(cnt.shape), cnt


class EvaluateVolume(EvaluateBase):
    """Evaluate a model case by case (volume by volume).

    volumes_on="device" keeps a case's volumes on the device from the raw crop to the metrics (see the module docstring);
    results are identical to "host".  It applies to --pred_type pred without --eval_in_patches: with --pred_type prob (an
    order-1 zoom of float volumes) or patches the evaluator silently takes the host path."""

    def __init__(self, estimator=None, model_dir=None, params=None, merge_tumor_to_liver=True, largest=True,
                 use_sg_reduce_fp=False, metrics_on="device", volumes_on="host"):
        super(EvaluateVolume, self).__init__()
        if metrics_on not in ("device", "host"):
            raise ValueError("metrics_on must be 'device' or 'host', got {!r}".format(metrics_on))
        if volumes_on not in ("device", "host"):
            raise ValueError("volumes_on must be 'device' or 'host', got {!r}".format(volumes_on))
        self.metrics_on = metrics_on
        self.volumes_on = volumes_on
        self.estimator = estimator
        self.model_dir = model_dir or (estimator.model_dir if estimator is not None else None)
        self.params = params or estimator.params
        self.config = self.params["args"]
        self.do_mirror = bool(getattr(self.config, "eval_mirror", False))
        self.mirror_variants, self.mirror_div = mirror_plan(self.config)
        self.merge_tumor_to_liver = merge_tumor_to_liver
        self.largest = largest
        self.use_sg_reduce_fp = bool(use_sg_reduce_fp and getattr(self.config, "use_spatial", False))
        self.eval_detection = bool(getattr(self.config, "eval_detection", False))
        self.detection_thresh = float(getattr(self.config, "detection_thresh", 0.5))
        if self.eval_detection and DETECTION_CLASS not in list(getattr(self.config, "classes", None) or []):
            raise ValueError("--eval_detection scores the {} class, which is not among --classes {}".format(
                DETECTION_CLASS, list(getattr(self.config, "classes", None) or [])))
        self.calls = 0
        self.seconds = 0.0
        self._saver = None                  # the _CaseSaver of a --save_predict run, while it runs
        self.save_join_each_case = False    # measurements: wait for each case's file instead of writing behind the next case

    @property
    def classes(self):
        return self.params["model_instances"][0].classes[1:]          # without background

    @property
    def metrics_str(self):
        return list(getattr(self.config, "metrics_eval", ["Dice"]))

    def _device_volumes(self, dtype=None):
        """Does this run keep its volumes on the device?  (volumes_on="device", class predictions, no patches.)"""
        dtype = dtype or getattr(self.config, "pred_type", "pred")
        return self.volumes_on == "device" and dtype == "pred" and not getattr(self.config, "eval_in_patches", False)

    def _zoom_back(self, volume, ori_shape, dtype):
        """Zoom a case's volume to ori_shape as the reference does (scipy.ndimage.zoom, order 0 for predictions and 1 for
        probabilities): a device tensor is zoomed on the device (predictions only), a numpy array on the host."""
        scales = np.array(ori_shape) / np.array(volume.shape)
        if not np.any(scales != 1):
            return volume
        if torch.is_tensor(volume):
            return ops.zoom_nearest3d(volume, ori_shape, ops.zoom_tables(tuple(volume.shape), ori_shape))
        return ndi.zoom(volume, scales, order=0 if dtype == "pred" else 1)

    # ------------------------------------------------------------------ device side
    def _model(self):
        if not self.params.get("model_instances"):
            self.params["model_instances"] = [self.params["model"](self.config)]
        return self.params["model_instances"][0]

    def _forward(self, model, features):
        inputs = {k: v for k, v in features.items() if torch.is_tensor(v) and k not in ("names",)}
        model(inputs, ModeKeys.EVAL, *self.params.get("model_args", ()), **self.params.get("model_kwargs", {}))
        return model.probability

    def _slab_probability(self, model, features):
        """Class probabilities of one slab, already divided by mirror_div; with device-side mirroring also averaged
        over the mirrored variants."""
        prob = self._forward(model, features)
        own_mirror = self.do_mirror and "mirror" not in features
        acc = torch.empty_like(prob)
        ops.flip_axpy(prob, acc, False, False, 1.0 / self.mirror_div, accumulate=False)
        if own_mirror:
            for m in self.mirror_variants:
                fh, fw = _FLIPS[m]
                flipped = dict(features)
                flipped["images"] = ops.flip_axpy(features["images"], None, fh, fw)
                if torch.is_tensor(features.get("sp_guide")):
                    flipped["sp_guide"] = ops.flip_axpy(features["sp_guide"], None, fh, fw)
                ops.flip_axpy(self._forward(model, flipped), acc, fh, fw, 1.0 / self.mirror_div, accumulate=True)
        return acc

    def _predict_case(self, predicts, cases=-1, dtype="pred", resize=False, save_path=None):
        """evaluator_liver.py:616-678 with the accumulation on the device.  Yields
        (case, segmentation, volume, post_processed); volume is a numpy array, or with _device_volumes a uint8 device
        tensor that was zoomed back on the device.  With save_path (--save_predict) the case is post-processed here, handed
        to the background writer (_maybe_save_case) and yielded as the post-processed class dict, post_processed = True."""
        on_device = self._device_volumes(dtype)
        slabs = []
        cur_case = None
        counter = 0
        for predict, labels in predicts:
            if predict is not None:
                new_case = str(predict["names"])
                cur_case = cur_case or new_case
                assert cur_case == new_case, (cur_case, new_case)
                m = int(predict.get("mirror", 0))
                if m == 0:
                    slabs.append(predict["Prob"])                       # already / mirror_div
                else:                                                   # a mirrored copy emitted by the pipeline
                    fh, fw = _FLIPS[m]
                    ops.flip_axpy(predict["Prob"], slabs[-1], fh, fw, 1.0, accumulate=True)
            else:
                assert isinstance(labels, tuple), type(labels)
                segmentation, vol_path, pads, bbox, reshape_ori = labels
                volume = torch.cat(slabs)                               # [d, h, w, c] on the device
                if pads > 0:
                    volume = volume[:-pads]
                if dtype == "pred":
                    amax, _ = ops.head_predict(volume.contiguous(), volume.shape[-1], want_preds=False)
                    volume = amax.view(volume.shape[:-1])               # np.argmax(volume, -1).astype(uint8)
                    if not on_device:
                        volume = volume.cpu().numpy()
                else:
                    volume = volume.cpu().numpy()
                if resize and reshape_ori:
                    ori_shape = (volume.shape[0],) + arr_ops.bbox_to_shape(bbox)[1:]
                    if volume.ndim == 4:
                        ori_shape = ori_shape + (volume.shape[-1],)
                    volume = self._zoom_back(volume, ori_shape, dtype)
                yield (cur_case, segmentation) + self._maybe_save_case(cur_case, volume, bbox, dtype, save_path)
                slabs.clear()
                cur_case = None
                counter += 1
                if 0 < cases <= counter:
                    break

    def _predict_case_patches(self, predicts, cases=-1, dtype="pred", save_path=None):
        """--eval_in_patches, evaluator_liver.py:524-566: window probabilities are written to their place in the liver
        box (a later window overwrites an earlier one where they overlap -- `result[...] = Prob`, :545 -- so the
        division by the coverage count the reference adds does not change the argmax and is not done), argmax on the
        device, labels cropped to the box.  The reference's run() hands this loop (preds, None) tuples it then indexes
        with strings (:537,763), i.e. its own path raises; this is the evident intent: labels travel with a case's
        last batch.  Yields like _predict_case."""
        result, covered = None, None
        counter = 0
        for predict, lab in predicts:
            bbox = predict["bbox"]
            prob = predict["Prob"]
            if result is None:
                shape = tuple(arr_ops.bbox_to_shape(bbox))
                result = torch.zeros(shape + (prob.shape[-1],), dtype=torch.float32, device=prob.device)
                covered = torch.zeros(shape, dtype=torch.bool, device=prob.device)
            positions = predict["position"]
            for i, (z, lb_y, ub_y, lb_x, ub_x) in enumerate(positions[:len(positions) - int(predict["pad"])]):
                result[z, lb_y:ub_y, lb_x:ub_x] = prob[i]
                covered[z, lb_y:ub_y, lb_x:ub_x] = True
            if lab is None:
                continue
            if not bool(covered.all()):
                raise RuntimeError("--eval_in_patches: windows do not cover the liver box of case {}".format(predict["name"]))
            segmentation = np.asarray(lab)[arr_ops.bbox_to_slices(bbox)].astype(np.uint8)
            if dtype == "pred":
                amax, _ = ops.head_predict(result.view(-1, result.shape[-1]), result.shape[-1], want_preds=False)
                volume = amax.view(result.shape[:-1]).cpu().numpy()
            else:
                volume = result.cpu().numpy()
            yield (str(predict["name"]), segmentation) + self._maybe_save_case(str(predict["name"]), volume, bbox, dtype,
                                                                               save_path)
            result, covered = None, None
            counter += 1
            if 0 < cases <= counter:
                break

    # ------------------------------------------------------------------ host side
    def _postprocess(self, volume, is_label=False, ori_shape=None):
        """evaluator_liver.py:680-702."""
        if not isinstance(volume, dict):
            decouple_volume = {cls: volume == i + 1 for i, cls in enumerate(self.classes)}
        else:
            decouple_volume = volume
        if ori_shape is not None:
            cur_shape = decouple_volume[self.classes[0]].shape
            ori_shape = [cur_shape[0]] + list(ori_shape)
            scales = np.array(ori_shape) / np.array(cur_shape)
            for cls in self.classes:
                decouple_volume[cls] = ndi.zoom(decouple_volume[cls], scales, order=0)
        if self.merge_tumor_to_liver and "Tumor" in decouple_volume and "Liver" in decouple_volume:
            decouple_volume["Liver"] = decouple_volume["Liver"] + decouple_volume["Tumor"]     # bool OR
        if self.largest and "Liver" in decouple_volume and not is_label:
            decouple_volume["Liver"] = arr_ops.get_largest_component(decouple_volume["Liver"], rank=3)
            if self.merge_tumor_to_liver and "Tumor" in decouple_volume:
                decouple_volume["Tumor"] = decouple_volume["Tumor"] * \
                    decouple_volume["Liver"].astype(decouple_volume["Tumor"].dtype)
        return decouple_volume

    def _postprocess_device(self, volume, is_label=False):
        """_postprocess on the device: `volume` is a device tensor of class ids (or a dict class -> device mask); returns
        class -> uint8 device mask, with tumor merged into liver and the liver reduced to its largest component."""
        if not isinstance(volume, dict):
            decouple_volume = {cls: (volume == i + 1).view(torch.uint8) for i, cls in enumerate(self.classes)}
        else:
            decouple_volume = dict(volume)
        if self.merge_tumor_to_liver and "Tumor" in decouple_volume and "Liver" in decouple_volume:
            decouple_volume["Liver"] = decouple_volume["Liver"] | decouple_volume["Tumor"]
        if self.largest and "Liver" in decouple_volume and not is_label:
            decouple_volume["Liver"] = ops.largest_component3d(decouple_volume["Liver"])
            if self.merge_tumor_to_liver and "Tumor" in decouple_volume:
                decouple_volume["Tumor"] = decouple_volume["Tumor"] & decouple_volume["Liver"]
        return decouple_volume

    def run_with_session(self, session=None):
        """evaluator_liver.py:164-169,286-330 (2-D): evaluate on the `eval_online` batches from inside training, with
        the live variables and moving statistics -- the mean of the in-graph "<Class>/<Metric>" values per batch, or
        with --use_global_dice the Dice of the summed confusion counts of the thresholded predictions."""
        if getattr(self.config, "eval_3d", False):
            return self._run_with_session_3d(session)
        model = self._model()
        if not getattr(self.config, "use_global_dice", False):
            keys = list(model.metrics_dict)
            acc = defaultdict(list)
            for x in self.estimator.evaluate_online(session, keys, yield_single_examples=False):
                for k, v in x.items():
                    acc[k].append(float(v))
            return {k: float(np.mean(v)) for k, v in acc.items()}
        acc = defaultdict(int)
        keys = ["labels"] + list(model.predictions)
        for x in self.estimator.evaluate_online(session, keys, yield_single_examples=False):
            labels = x["labels"].cpu().numpy()
            for i, cls in enumerate(self.classes):
                pred = np.squeeze(x[cls + "Pred"].cpu().numpy(), axis=-1).astype(int)
                conf = metric_ops.ConfusionMatrix(pred, (labels == i + 1).astype(int))
                conf.compute()
                acc[cls + "_fn"] += conf.fn
                acc[cls + "_fp"] += conf.fp
                acc[cls + "_tp"] += conf.tp
        return {cls + "/Dice": 2 * acc[cls + "_tp"] / max(2 * acc[cls + "_tp"] + acc[cls + "_fn"] + acc[cls + "_fp"], 1)
                for cls in self.classes}

    def _run_with_session_3d(self, session=None):
        """evaluator_liver.py:171-282 (--eval_3d): the `eval_online` pipeline serves every validation case as consecutive
        slice batches over the liver's z range (data/lits.batches_eval_3d); the thresholded predictions of a case are
        stacked, the padding slices of its last batch dropped, and each class volume is scored against (labels == class)
        -- per-case `metric_3d` averaged over the cases, or with --use_global_dice the Dice of the confusion counts summed
        over all cases.  No post-processing (the reference omits it here to save training time, :208-210).
        The volumes stay on the device until a case is complete: one device->host copy per case.
        (The reference's per-case branch indexes the label ARRAY with the class name, :212,:234 -- it cannot run as written;
        this restates the evident intent, the same comparison its global-Dice branch makes at :262.)"""
        model = self._model()
        keys = ["labels", "names"] + list(model.predictions)
        use_global = bool(getattr(self.config, "use_global_dice", False))
        self.clear_metrics()
        acc = defaultdict(int)
        depths = {}
        for fold_case in self.params.get(("lits_store", False), (None, []))[1]:
            depths[str(int(fold_case["PID"]))] = int(fold_case["bbox"][3] - fold_case["bbox"][0])

        def finish(case, preds, labels):
            vol = {cls: torch.cat(preds[cls], dim=0) for cls in self.classes}
            lab = torch.cat(labels, dim=0)
            n_real = depths.get(case, lab.shape[0])                    # drop the padding slices of the last batch
            if self.metrics_on == "device":
                return finish_device(vol, lab[:n_real], n_real)
            lab = lab[:n_real].cpu().numpy()
            results = {}
            for i, cls in enumerate(self.classes):
                pred = vol[cls][:n_real].cpu().numpy().astype(np.uint8)
                ref = (lab == i + 1).astype(np.uint8)
                if self.eval_detection and cls == DETECTION_CLASS:
                    self._add_detection(acc, metric_ops.tumor_detection_metrics(pred, ref, self.detection_thresh))
                if use_global:
                    conf = metric_ops.ConfusionMatrix(pred.astype(int), ref.astype(int))
                    conf.compute()
                    acc[cls + "_fn"] += conf.fn
                    acc[cls + "_fp"] += conf.fp
                    acc[cls + "_tp"] += conf.tp
                else:
                    for met, value in metric_ops.metric_3d(pred, ref, required=self.metrics_str).items():
                        results["{}/{}".format(cls, met)] = value
            if not use_global:
                self.append_metrics(results)

        def finish_device(vol, lab, n_real):
            results = {}
            for i, cls in enumerate(self.classes):
                pred = vol[cls][:n_real].to(torch.uint8)
                ref = (lab == i + 1).view(torch.uint8)
                if self.eval_detection and cls == DETECTION_CLASS:
                    self._add_detection(acc, metric_ops.tumor_detection_metrics_device(pred, ref, self.detection_thresh))
                if use_global:
                    conf = ops.mask_counts(pred, ref)
                    acc[cls + "_fn"] += conf["fn"]
                    acc[cls + "_fp"] += conf["fp"]
                    acc[cls + "_tp"] += conf["tp"]
                else:
                    for met, value in metric_ops.metric_3d_device(pred, ref, required=self.metrics_str).items():
                        results["{}/{}".format(cls, met)] = value
            if not use_global:
                self.append_metrics(results)

        cur, preds, labels = None, defaultdict(list), []
        for x in self.estimator.evaluate_online(session, keys, yield_single_examples=False):
            case = str(int(x["names"][0]))
            if cur is not None and case != cur:
                finish(cur, preds, labels)
                preds, labels = defaultdict(list), []
            cur = case
            for cls in self.classes:
                preds[cls].append(x[cls + "Pred"].reshape(x[cls + "Pred"].shape[:3]))
            labels.append(x["labels"])
        if cur is not None:
            finish(cur, preds, labels)
        if use_global:
            results = {cls + "/Dice": 2 * acc[cls + "_tp"] / max(2 * acc[cls + "_tp"] + acc[cls + "_fn"] + acc[cls + "_fp"], 1)
                       for cls in self.classes}
        else:
            results = {k: float(np.mean(v)) for k, v in self.metric_values.items()}
        if self.eval_detection:                                         # per case, on the volumes as they are scored here
            results.update(self._detection_results(acc))
        return results

    def run(self, input_fn, checkpoint_path=None, latest_filename=None, save=False, hooks=None, cases=None):
        """evaluator_liver.py:704-766: build the model, restore the checkpoint, stream the cases."""
        model = self._model()
        restored = [False]
        # a requested checkpoint must exist -- a TensorFlow V2 prefix (`model.ckpt-3` = .index + .data-* files) or a file of
        # this package; the reference raises FileNotFoundError (:705-708).  checkpoint_path=None scores the live variables.
        if checkpoint_path and not tf_checkpoint.checkpoint_exists(checkpoint_path):
            raise FileNotFoundError("Missing checkpoint file {} (status_file {})".format(checkpoint_path, latest_filename))
        mode = getattr(self.config, "mode", ModeKeys.EVAL)
        patches = bool(getattr(self.config, "eval_in_patches", False))

        params = dict(self.params, volumes_on="device") if self._device_volumes() else self.params

        def run_pred():
            for features, labels in input_fn(mode, params):
                if features:
                    # host generators (the reference's contract: numpy slabs, data/lits.input_fn_eval) -> one upload per slab
                    features = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v)
                                for k, v in features.items()}
                    if not restored[0]:
                        restored[0] = True
                        if model.params is None:
                            self._forward(model, features)              # creates the variables
                        if checkpoint_path and self.estimator is not None:
                            self.estimator._restore(checkpoint_path, model, None)
                    preds_eval = {k: v for k, v in features.items() if not torch.is_tensor(v) or k == "names"}
                    preds_eval["Prob"] = self._slab_probability(model, features)
                    yield preds_eval, (labels if patches else None)
                else:
                    yield None, labels

        n_cases = cases if cases is not None else getattr(self.config, "eval_num", -1)
        if patches:
            return self._run_actual(self._predict_case_patches, run_pred, save, cases=n_cases)
        resize = getattr(self.config, "im_height", 0) > 0 and getattr(self.config, "im_width", 0) > 0
        return self._run_actual(self._predict_case, run_pred, save, cases=n_cases, resize=resize)

    # ------------------------------------------------------------------ UNet3D in sliding windows
    def run_3d(self, input_fn, checkpoint_path=None, save=False, cases=None):
        """Whole LiTS cases scored by UNet3D in sliding windows (`liver_3d --mode eval --eval_in_patches`; the reference's
        evaluators/evaluator_nf.py:194-257 `_evaluate_patches`).  input_fn: data/lits3d.input_fn_eval --
        per case the host tables of its windows, then an end-of-case item.  Per table: one pinned upload, the windows cut by
        `unetk_lits_patch3d` as `eval_online` cuts them, one forward, and `unetk_eval3d_accumulate`, which resizes the window
        probabilities back to their crops and ADDS them into the case's accumulator at source resolution (the reference
        assigns but counts: its last window is divided by the coverage).  At the end of a case: argmax over the sums (the
        division by a positive count does not change it), labels from the resident store, and the usual post-processing
        and metrics on the device.  Nothing inside a case synchronises the host; the coverage count is read once per case.
        --eval_window_weight gaussian: the windows are added with the per-axis tables of lits3d.window_weights
        (`unetk_eval3d_accumulate_w`, a float weight volume for the count).  --eval_box_from: the case's windows tile a box only
        (the end-of-case item carries it) and everything outside it is class 0.  With either flag `unetk_eval3d_finish` is
        the argmax inside the box (the whole case without --eval_box_from) and counts the box's voxels without cover; the
        count is read where the plain path reads cnt.min()."""
        cfg = self.config
        model = self._model()
        if checkpoint_path and not tf_checkpoint.checkpoint_exists(checkpoint_path):
            raise FileNotFoundError("Missing checkpoint file {} (status_file None)".format(checkpoint_path))
        mode = getattr(cfg, "mode", ModeKeys.EVAL)
        params = self.params
        from ..data import lits3d
        lits3d.label_map(cfg.classes)                                   # refuses other --classes than the LiTS label maps
        windows = CaseWindows3D(lambda features: self._forward(model, features), cfg)
        restored = [False]

        def restore_once(features):
            if not restored[0]:
                restored[0] = True
                if model.params is None:
                    self._forward(model, features)                      # creates the variables
                if checkpoint_path and self.estimator is not None:
                    self.estimator._restore(checkpoint_path, model, None)

        do_eval = mode not in ("predict", ModeKeys.PREDICT)
        want_prob = getattr(cfg, "pred_type", "pred") == "prob"

        def run_pred():
            for tab, end in input_fn(mode, params):
                if tab is not None:
                    # --mode infer: the table's own one-case store; else the fold's, resident before input_fn_eval's first item
                    # --z_spacing: the item beside a table carries the case's crop depth
                    store = end["store"] if end is not None and "store" in end else params[("lits_store", False)][0]
                    windows.add(store, tab, before_forward=restore_once, zcrop=end.get("zcrop") if end is not None else None)
                else:
                    if windows.acc is None or end["depth"] != windows.acc.shape[0]:
                        raise RuntimeError("case {} ended without windows of its own".format(end["case"]))
                    if self._saver is not None and end.get("header") is not None:
                        self._saver.given[str(end["case"])] = (end["header"], bool(end.get("special", False)))
                    # --mode infer makes no label request: there is nothing to score
                    labels = windows.labels(end["store"], end["base"], end["depth"]) if do_eval else None
                    volume, cover = windows.finish(end.get("box"), keep=want_prob)
                    probs = None
                    if want_prob:
                        probs = windows.kept + (end.get("box"),)
                        windows.kept = None
                    yield end["case"], labels, volume, cover, probs

        n_cases = cases if cases is not None else getattr(cfg, "eval_num", -1)
        return self._run_actual(self._predict_case_3d, run_pred, save, cases=n_cases)

    def _predict_case_3d(self, predicts, cases=-1, dtype="pred", save_path=None):
        """A case of run_3d for _run_actual: (case, device labels, device class volume uint8 [depth, src_h, src_w], False).
        The coverage is read here, where the scoring that follows synchronises anyway.  With save_path the volume is saved as
        in _predict_case, its box being the whole case at source resolution.  --pred_type prob: the class volume is still what
        is yielded (and scored in --mode eval); what is saved is one `prob-<case>-<Class>.nii.gz` per foreground class instead
        (`unetk_eval3d_prob` on the case's accumulator, _CaseSaver.save_prob)."""
        counter = 0
        for case, labels, volume, cnt, probs in predicts:
            # cnt: the coverage volume [depth, src_h, src_w] of the plain path, or the word [1] eval3d_finish counted into
            if (int(cnt.item()) != 0) if cnt.dim() == 1 else (int(cnt.min().item()) <= 0):
                raise RuntimeError("--eval_in_patches: windows do not cover every voxel of case {}".format(case))
            depth, src_h, src_w = (int(v) for v in volume.shape)
            if dtype != "pred":
                if save_path is not None and self._saver is not None:
                    self._saver.save_prob(str(case), *probs)
                yield case, labels, volume, False
            else:
                yield (case, labels) + self._maybe_save_case(case, volume, (0, 0, 0, src_w - 1, src_h - 1, depth - 1), dtype,
                                                             save_path)
            counter += 1
            if 0 < cases <= counter:
                break

    # ------------------------------------------------------------------ spatial-guide propagation
    def run_g(self, input_fn=None, checkpoint_path=None, latest_filename=None, save=False, cases=None, timing=None,
              trace=None):
        """evaluator_liver.py:818-917 with --use_spatial: every case of the validation fold is walked slice by slice up and
        then down, each slice guided by the prior and by the tumours predicted on the previous one (data/propagate.py).
        Per slice on the device: one forward over the image, its mirrors and the guide's mirrors, the mirror-averaged
        probabilities written into the case's resident slot of the sweep, `unetk_guide_components`, one small table copied
        to pinned host memory (the slice's only sync; the head and 256 rows, the rest only for a slice with more components),
        the host's matching, and `unetk_guide_render` for the next slice.
        The two sweeps' volumes are combined as max(forward, flip_z(backward)) on the device, then argmax, zoom back to the
        box (order 0) and the usual post-processing and metrics.  timing (a dict): per-phase seconds, measured with a device
        sync between phases (for measurements only).  trace (a list): receives per slice (direction, sid, objects,
        components at or above the threshold, their decisions, number of components below it)."""
        from ..data import lits, propagate
        cfg = self.config
        if getattr(cfg, "save_sp_guide", False):
            raise NotImplementedError("--save_sp_guide is not supported by the propagated evaluation")
        if getattr(cfg, "mode", ModeKeys.EVAL) == ModeKeys.PREDICT:
            raise NotImplementedError("--mode predict with --use_spatial is not supported (the evaluation needs labels)")
        if checkpoint_path and not tf_checkpoint.checkpoint_exists(checkpoint_path):
            raise FileNotFoundError("Missing checkpoint file {} (status_file {})".format(checkpoint_path, latest_filename))
        root = self.params["lits_root"]
        data = lits.collect_datasets(root, cfg.test_fold, "eval", filter_tumor_size=getattr(cfg, "filter_size", 0),
                                     filter_only_liver_in_val=self.params.get("filter_only_liver_in_val", True))
        if len(data) == 0:
            raise ValueError("No valid dataset found!")
        context = None
        if getattr(cfg, "use_context", False):
            context = lits.EvalContext(root, lits.context_list_from_args(cfg),
                                       float(getattr(cfg, "hist_scale", 20.)), self.params.get("device"))
        prior = propagate.load_prior(root, getattr(cfg, "real_sp", None))
        state = propagate.Propagation(prior, float(getattr(cfg, "min_std", 2.)), float(getattr(cfg, "eval_discount", 0.85)),
                                      (cfg.im_height, cfg.im_width))
        source = propagate.EvalCases(data, cfg, self.params.get("proj_root", "."), root, context)
        model = self._model()

        def run_pred():
            loop = _GuidedLoop(self, model, state, checkpoint_path, timing, trace)
            for item in source:
                yield item, loop.case(item)

        n_cases = cases if cases is not None else -1
        return self._run_actual(self._predict_case_g, run_pred, save, cases=n_cases)

    def _predict_case_g(self, predicts, cases=-1, dtype="pred", save_path=None):
        """evaluator_liver.py:768-816: the combined probability volume of a case (already max(forward, flip_z(backward)) on
        the device) -> argmax (or the probabilities with --pred_type prob) -> zoom back to the box (on the device with
        _device_volumes, like _predict_case)."""
        on_device = self._device_volumes(dtype)
        counter = 0
        for item, volume in predicts:
            if dtype == "pred":
                amax, _ = ops.head_predict(volume.view(-1, volume.shape[-1]), volume.shape[-1], want_preds=False)
                volume = amax.view(volume.shape[:-1])
                if not on_device:
                    volume = volume.cpu().numpy()
            else:
                volume = volume.cpu().numpy()
            ori_shape = (volume.shape[0],) + arr_ops.bbox_to_shape(item["bbox"])[1:]
            if volume.ndim == 4:
                ori_shape = ori_shape + (volume.shape[-1],)
            volume = self._zoom_back(volume, ori_shape, dtype)
            yield (str(item["pid"]), item["segmentation"]) + self._maybe_save_case(str(item["pid"]), volume, item["bbox"],
                                                                                   dtype, save_path)
            counter += 1
            if 0 < cases <= counter:
                break

    def _run_actual(self, predict_fn, run_fn, save, cases=-1, **run_kwargs):
        """evaluator_liver.py:906-996; returns the averaged results (the reference only logs them)."""
        do_eval = getattr(self.config, "mode", ModeKeys.EVAL) not in ("predict", ModeKeys.PREDICT)
        save_path = None
        if save:
            save_path = Path(self.model_dir) / (getattr(self.config, "save_path", None) or "prediction")
            save_path.mkdir(parents=True, exist_ok=True)
            self._saver = _CaseSaver(self, save_path)
        elif not do_eval:
            log.warning("--mode infer without --save_predict: the predictions are computed and nothing is written")
        try:
            results = self._run_cases(predict_fn, run_fn, save_path, do_eval, cases, **run_kwargs)
            if self._saver is not None:
                self._saver.writer.close()                              # every file is complete before results.json says so
        except BaseException:
            if self._saver is not None:
                self._saver.abandon()
            raise
        finally:
            self._saver = None
        if save_path is not None:
            with (save_path / "results.json").open("w") as f:
                json.dump(results, f)
        return results

    def _run_cases(self, predict_fn, run_fn, save_path, do_eval, cases=-1, **run_kwargs):
        """The loop of _run_actual over the cases."""
        accumulator = defaultdict(int)
        use_global = bool(getattr(self.config, "use_global_dice", False))
        self.clear_metrics()
        self.calls, self.seconds = 0, 0.0
        tic = time.perf_counter()
        for cur_case, labels, volume, post_processed in predict_fn(run_fn(), cases=cases,
                                                                   dtype=getattr(self.config, "pred_type", "pred"),
                                                                   save_path=save_path, **run_kwargs):
            results = {}
            if do_eval and self.metrics_on == "device":
                self._score_case_device(volume, labels, post_processed, accumulator, use_global)
            elif do_eval:
                if torch.is_tensor(volume):                             # volumes_on="device" with the host metrics
                    volume = volume.cpu().numpy()
                if not post_processed:
                    volume = self._postprocess(volume)
                labels = self._postprocess(labels, is_label=True)
                for cls in self.classes:
                    conf = metric_ops.ConfusionMatrix(volume[cls].astype(int), labels[cls].astype(int))
                    conf.compute()
                    accumulator[cls + "_fn"] += conf.fn
                    accumulator[cls + "_fp"] += conf.fp
                    accumulator[cls + "_tp"] += conf.tp
                if self.eval_detection:
                    self._add_detection(accumulator, metric_ops.tumor_detection_metrics(
                        volume[DETECTION_CLASS], labels[DETECTION_CLASS], self.detection_thresh))
                if not use_global:
                    for cls in self.classes:
                        pairs = metric_ops.metric_3d(volume[cls], labels[cls], required=self.metrics_str)
                        for met, value in pairs.items():
                            results["{}/{}".format(cls, met)] = value
                    self.append_metrics(results)
            if self._saver is not None and self.save_join_each_case:
                self._saver.writer.join()
            self.calls += 1
            self.seconds += time.perf_counter() - tic
            tic = time.perf_counter()
        if not do_eval:
            return {}

        def gdice(cls):
            den = 2 * accumulator[cls + "_tp"] + accumulator[cls + "_fn"] + accumulator[cls + "_fp"]
            return 2 * accumulator[cls + "_tp"] / den if den else 0.0

        if use_global:
            results = {cls + "Dice": gdice(cls) for cls in self.classes}
        else:
            results = {key: float(np.mean(values)) for key, values in self._metric_values.items()}
            if accumulator:
                results.update({"G" + cls + "Dice": gdice(cls) for cls in self.classes})
        if self.eval_detection:
            results.update(self._detection_results(accumulator))
        return results

    @staticmethod
    def _add_detection(accumulator, det):
        """One case's tumor_detection_metrics into the run's counts."""
        accumulator[DETECTION_CLASS + "_det_tp"] += det["tp"]
        accumulator[DETECTION_CLASS + "_det_fp"] += det["fp"]
        accumulator[DETECTION_CLASS + "_det_pos"] += det["pos"]

    @staticmethod
    def _detection_results(accumulator):
        """--eval_detection: the counts summed over the cases, and precision / recall of the sums (np.inf where the
        denominator is 0, as per case)."""
        tp, fp, pos = (int(accumulator[DETECTION_CLASS + "_det_" + k]) for k in ("tp", "fp", "pos"))
        scores = metric_ops.detection_scores(tp, tp + fp, pos)
        return {DETECTION_CLASS + "/DetTP": tp, DETECTION_CLASS + "/DetFP": fp, DETECTION_CLASS + "/DetPos": pos,
                DETECTION_CLASS + "/Precision": float(scores["precision"]), DETECTION_CLASS + "/Recall": float(scores["recall"])}

    def _maybe_save_case(self, case, volume, bbox, dtype, save_path):
        """evaluator_liver.py:998-1026 `maybe_save_case`: -> (volume, post_processed).  Without --save_predict the volume
        passes through; with it, see _CaseSaver.save."""
        if save_path is None or self._saver is None:
            return volume, False
        return self._saver.save(str(case), volume, bbox, dtype)

    def _score_case_device(self, volume, labels, post_processed, accumulator, use_global):
        """One case of _run_actual on the device: one upload of the volume (none when it is a device tensor already:
        volumes_on="device") and one of the labels, then post-processing, the global Dice counts and metric_3d_device per
        class."""
        def upload(x):
            return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
        if post_processed:
            volume = {cls: upload(v) for cls, v in volume.items()}
        else:
            volume = self._postprocess_device(upload(volume))
        labels = self._postprocess_device(upload(labels), is_label=True)
        results = {}
        for cls in self.classes:
            conf = ops.mask_counts(volume[cls], labels[cls])
            accumulator[cls + "_fn"] += conf["fn"]
            accumulator[cls + "_fp"] += conf["fp"]
            accumulator[cls + "_tp"] += conf["tp"]
        if self.eval_detection:
            self._add_detection(accumulator, metric_ops.tumor_detection_metrics_device(
                volume[DETECTION_CLASS], labels[DETECTION_CLASS], self.detection_thresh))
        if not use_global:
            for cls in self.classes:
                for met, value in metric_ops.metric_3d_device(volume[cls], labels[cls], required=self.metrics_str).items():
                    results["{}/{}".format(cls, met)] = value
            self.append_metrics(results)

    def compare(self, *args_, **kwargs):
        return _compare(*args_, **kwargs)


class _CaseSaver(object):
    """--save_predict for one run of EvaluateVolume: `<save_path>/predict-<case>.nii.gz` holds the post-processed
    Liver + Tumor mask of the case, padded from its box to the whole volume, with the header of the case's own volume file
    (evaluator_liver.py:998-1026); --pred_type prob writes `<case>.npz` with the zero-padded 4-D probabilities instead.

    A volume that is on the device and scored there (volumes_on = metrics_on = "device", and run_3d) is post-processed by
    _postprocess_device, composed in file order by `unetk_nii_compose` and copied once; otherwise the reference's host
    path (np.pad, write_nii's flips and transpose) runs in the writer thread.  Both write the same bytes.  The files are
    written by utils/volume_writer.VolumeWriter behind the evaluation of the next case.

    Header: what the input function handed in for the case (`given`: liver_3d --mode infer, the input file's own), else the
    case's `vol_case` of meta.json under params["proj_root"], read header-only; when the entry or the file is
    missing (the PNG store of liver_3d needs no NIfTI), nii_kits.header_from_meta of its `size` and `spacing`, logged once.
    Unlike the reference, which calls write_nii without `special`, the write inverts the read: cases 28..47 are x-mirrored
    as read_lits("vol") mirrors them, so voxel (i, j, k) of the written file is voxel (i, j, k) of the volume file."""

    def __init__(self, evaluator, save_path):
        from ..utils.volume_writer import VolumeWriter
        self.ev, self.save_path = evaluator, Path(save_path)
        self.writer = VolumeWriter()
        self._meta = None
        self._told_fallback = False
        self.given = {}                 # case -> (header, special) handed in by the input function (liver_3d --mode infer)

    def abandon(self):
        """The way out of an exception: stop the thread; what it met is second to the exception under way."""
        try:
            self.writer.close()
        except Exception as err:         # noqa: the first exception is the one to report
            log.error("the volume writer failed as well: %r", err)

    def _case_meta(self, pid):
        if self._meta is None:
            root = self.ev.params.get("lits_root")
            self._meta = {}
            if root is not None and (Path(root) / "meta.json").exists():
                with (Path(root) / "meta.json").open() as f:
                    self._meta = {int(c["PID"]): c for c in json.load(f)}
        return self._meta.get(pid)

    def header(self, case):
        """(header, special) of a case; special = the x mirror of read_lits("vol")."""
        from ..data import nii_kits
        from ..data.lits import _maybe_json
        if str(case) in self.given:                                   # the input file's own header comes first
            return self.given[str(case)]
        pid = int(case)
        meta = self._case_meta(pid)
        if meta is None:
            raise ValueError("--save_predict: case {} is not in meta.json of {}".format(case, self.ev.params.get("lits_root")))
        special = 28 <= pid < 48
        vol_case = meta.get("vol_case")
        if vol_case:
            path = Path(self.ev.params.get("proj_root", ".")) / vol_case
            if path.exists():
                return nii_kits.load_header(path), special
        if not self._told_fallback:
            self._told_fallback = True
            log.info("--save_predict: no volume file for case %s (vol_case %r); headers are built from meta.json's size and "
                     "spacing", case, vol_case)
        return nii_kits.header_from_meta(_maybe_json(meta["size"]), _maybe_json(meta["spacing"])), special

    def save_prob(self, case, acc, weight, box=None):
        """--pred_type prob of the sliding-window 3-D path: one `prob-<case>-<Class>.nii.gz` per foreground class, uint8
        q = rint(255 p) in the case's file order with scl_slope = 1 / 255 (nii_kits.prob_header), composed on the device by
        `unetk_eval3d_prob` from the case's accumulator and written by the same thread."""
        from ..data import nii_kits
        header, special = self.header(case)
        case_shape = nii_kits.data_shape(header)
        if tuple(acc.shape[:3]) != tuple(case_shape):
            raise ValueError("--save_predict: the accumulator of case {} has shape {}, its volume {}".format(
                case, tuple(acc.shape[:3]), case_shape))
        trans_bk, flips = nii_kits.file_orientation(header, special)
        file_shape = tuple(case_shape[axis] for axis in trans_bk)
        out_header = nii_kits.prob_header(header)
        for i, cls in enumerate(self.ev.classes):
            flat = ops.eval3d_prob(acc, weight, i + 1, box, trans_bk, flips)
            self.writer.submit(self.save_path / "prob-{}-{}.nii.gz".format(case, cls), out_header, file_shape, flat)

    def save(self, case, volume, bbox, dtype):
        from ..data import nii_kits
        header, special = self.header(case)
        case_shape = nii_kits.data_shape(header)
        origin = (int(bbox[2]), int(bbox[1]), int(bbox[0]))
        box = tuple(arr_ops.bbox_to_shape(bbox))
        if tuple(volume.shape[:3]) != box:
            raise ValueError("--save_predict: the volume of case {} has shape {}, its box {} (evaluate with the resize back "
                             "to the box)".format(case, tuple(volume.shape[:3]), box))
        if any(o < 0 or o + b > n for o, b, n in zip(origin, box, case_shape)):
            raise ValueError("--save_predict: the box {} at {} of case {} leaves its volume {}".format(
                box, origin, case, case_shape))
        pad_with = tuple((o, n - o - b) for o, b, n in zip(origin, box, case_shape))
        if dtype != "pred":                                           # the 4-D probabilities -> <case>.npz
            save_file = self.save_path / (case + ".npz")
            self.writer.submit_call(save_file, lambda: np.savez_compressed(
                str(save_file), np.pad(volume, pad_with + ((0, 0),), mode="constant", constant_values=0)))
            return volume, False
        save_file = self.save_path / "predict-{}.nii.gz".format(case)
        trans_bk, flips = nii_kits.file_orientation(header, special)
        file_shape = tuple(case_shape[axis] for axis in trans_bk)
        if torch.is_tensor(volume) and self.ev.metrics_on == "device":
            volume = self.ev._postprocess_device(volume)
            if "Liver" not in volume and "Tumor" not in volume:
                raise ValueError("Not supported save object!")
            flat = ops.nii_compose(volume.get("Liver"), volume.get("Tumor"), origin, case_shape, trans_bk, flips)
            self.writer.submit(save_file, header, file_shape, flat)
            return volume, True
        if torch.is_tensor(volume):
            volume = volume.cpu().numpy()
        volume = self.ev._postprocess(volume)
        parts = [np.asarray(volume[cls]).astype(np.uint8) for cls in ("Liver", "Tumor") if cls in volume]
        if not parts:
            raise ValueError("Not supported save object!")
        img_array = parts[0] + parts[1] if len(parts) == 2 else parts[0]

        def write():
            padded = np.pad(img_array, pad_with, mode="constant", constant_values=0)
            nii_kits.save_flat(nii_kits.to_file_order(padded, header, special), file_shape, header, save_file)
        self.writer.submit_call(save_file, write)
        return volume, True


GUIDE_TABLE_CAP = 16384         # components per slice the device table holds (more raise): an early checkpoint can predict
#                                 thousands of specks
GUIDE_TABLE_FIRST = 256         # rows copied with the head every slice (12 KB); more are fetched only when a slice has more


class _GuidedLoop(object):
    """The device side of EvaluateVolume.run_g: buffers that live across slices and cases, and one case at a time."""

    def __init__(self, evaluator, model, state, checkpoint_path, timing=None, trace=None):
        from ..data import propagate
        self.ev, self.model, self.state, self.ckpt = evaluator, model, state, checkpoint_path
        self.propagate = propagate
        self.timing, self.trace = timing, trace
        cfg = evaluator.config
        self.h, self.w, self.c = int(cfg.im_height), int(cfg.im_width), int(cfg.im_channel)
        self.variants = list(evaluator.mirror_variants)
        self.scale = 1.0 / evaluator.mirror_div
        self.dev = torch.device("cuda", torch.cuda.current_device())
        b = 1 + len(self.variants)
        self.images = torch.empty((b, self.h, self.w, self.c), dtype=torch.float32, device=self.dev)
        self.sp = torch.empty((b, self.h, self.w, 1), dtype=torch.float32, device=self.dev)
        self.guide = torch.empty((self.h, self.w), dtype=torch.float32, device=self.dev)
        self.table = torch.empty(4 + GUIDE_TABLE_CAP * ops.GUIDE_ROW, dtype=torch.int32, device=self.dev)
        self.table_host = torch.empty(self.table.shape, dtype=torch.int32, pin_memory=True)
        self.obj_host = torch.empty((64, 4), dtype=torch.float32, pin_memory=True)
        self.obj = torch.empty((64, 4), dtype=torch.float32, device=self.dev)
        self.ws = ops.guide_components_ws(self.h, self.w, GUIDE_TABLE_CAP, self.dev)
        self.restored = False
        self._tic = None

    def _mark(self, phase):
        """timing only: charge the time since the previous mark to `phase`, with the device idle at both ends."""
        if self.timing is None:
            return
        torch.cuda.synchronize()
        now = time.perf_counter()
        if phase is not None and self._tic is not None:
            self.timing[phase] = self.timing.get(phase, 0.0) + now - self._tic
        self._tic = now

    def _render(self, objects):
        n = len(objects)
        if n > self.obj.shape[0]:
            cap = max(n, 2 * self.obj.shape[0])
            self.obj_host = torch.empty((cap, 4), dtype=torch.float32, pin_memory=True)
            self.obj = torch.empty((cap, 4), dtype=torch.float32, device=self.dev)
        if n:
            self.obj_host[:n].numpy()[:] = objects
            self.obj[:n].copy_(self.obj_host[:n], non_blocking=True)       # the previous slice's sync freed obj_host
        ops.guide_render(self.obj[:n] if n else None, (self.h, self.w), self.state.discount, out=self.guide)

    def _forward(self, feats):
        if not self.restored:
            self.restored = True
            if self.model.params is None:
                self.ev._forward(self.model, feats)                            # creates the variables
            if self.ckpt and self.ev.estimator is not None:
                self.ev.estimator._restore(self.ckpt, self.model, None)
        return self.ev._forward(self.model, feats)

    def case(self, item):
        """The combined class probabilities [d, H, W, 3] of one case on the device."""
        cshape, lhc, rhc, bbox = item["cshape"], item["lhc"], item["rhc"], item["bbox"]
        depth = cshape[0] - lhc - rhc
        vol = torch.from_numpy(np.ascontiguousarray(np.moveaxis(item["volume"], -1, 0))).to(self.dev)    # [z, H, W]
        ctx = item["context"]
        fwd = torch.empty((depth, self.h, self.w, 3), dtype=torch.float32, device=self.dev)
        bwd = torch.empty_like(fwd)
        for direction, idx in self.propagate.sweeps(cshape, lhc, rhc):
            zz1 = idx - lhc
            sid = zz1 + bbox[2]
            self._mark(None)
            objects = self.state.start_slice(item["pid"], sid, bbox, cshape)
            self._render(objects)
            self._mark("render")
            self.images[0].copy_(vol[zz1:zz1 + self.c].permute(1, 2, 0))
            self.sp[0, :, :, 0].copy_(self.guide)
            for j, m in enumerate(self.variants):
                fh, fw = _FLIPS[m]
                ops.flip_axpy(self.images[0:1], self.images[j + 1:j + 2], fh, fw)
                ops.flip_axpy(self.sp[0:1], self.sp[j + 1:j + 2], fh, fw)
            feats = {"images": self.images, "sp_guide": self.sp}
            if ctx is not None:
                feats["context"] = ctx[sid:sid + 1].expand(self.images.shape[0], -1).contiguous()
            prob = self._forward(feats)
            slot = (fwd if direction == "Forward" else bwd)[zz1:zz1 + 1]       # backward slices land flipped back in z
            ops.flip_axpy(prob[0:1], slot, False, False, self.scale, accumulate=False)
            for j, m in enumerate(self.variants):
                fh, fw = _FLIPS[m]
                ops.flip_axpy(prob[j + 1:j + 2], slot, fh, fw, self.scale, accumulate=True)
            self._mark("forward")
            ops.guide_components(slot[0], self.guide, GUIDE_TABLE_CAP, table=self.table, ws=self.ws)
            self._mark("components")
            head = 4 + GUIDE_TABLE_FIRST * ops.GUIDE_ROW
            self.table_host[:head].copy_(self.table[:head], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            count = int(self.table_host[0])
            if GUIDE_TABLE_FIRST < count <= GUIDE_TABLE_CAP:          # a speckled slice: the rest of its rows
                end = 4 + count * ops.GUIDE_ROW
                self.table_host[head:end].copy_(self.table[head:end], non_blocking=True)
                torch.cuda.current_stream().synchronize()
            comps, n_low = self.propagate.parse_table(self.table_host.numpy(), self.w, skip_low=True)
            decisions = self.state.finish_slice(sid, comps, lambda: self.guide.cpu().numpy(), n_low)
            self._mark("sync_match")
            if self.trace is not None:
                self.trace.append((direction, sid, objects, comps, decisions, n_low))
        torch.maximum(fwd, bwd, out=fwd)
        return fwd


def _compare(cur_result, ori_result, primary_metric=None, secondary_metric=None):
    """Is `cur_result` better than `ori_result`?  (evaluator_liver.py:1193-1227)  Larger is better for every metric; the
    results are ranked lexicographically with the primary metric first, the secondary second, then the remaining keys in
    the dict's own order; a complete tie is "not better".  Same argument errors as the reference."""
    for name, res in (("cur_result", cur_result), ("ori_result", ori_result)):
        if not isinstance(res, dict):
            raise TypeError("`{}` should be dict, but got {}".format(name, type(res)))
    if set(cur_result) != set(ori_result):
        raise ValueError("Dicts with different keys can not be compared. cur_result({}) vs ori_result({})"
                         .format(list(cur_result.keys()), list(ori_result.keys())))
    for name, key in (("primary_metric", primary_metric), ("secondary_metric", secondary_metric)):
        if key and key not in cur_result:
            raise KeyError("`{}` not in valid result key: {}".format(name, key))
    if primary_metric == secondary_metric:
        raise ValueError("`primary_metric` can not be equal to `secondary_metric`")
    lead = [primary_metric] + ([secondary_metric] if secondary_metric else []) if primary_metric else []
    order = lead + [k for k in cur_result if k not in lead]
    return tuple(cur_result[k] for k in order) > tuple(ori_result[k] for k in order)
