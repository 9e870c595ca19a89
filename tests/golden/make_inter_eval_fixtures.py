"""Interactive-evaluation fixtures pinned on the REFERENCE ITSELF (build container only): entry/main_eval.py's
`inter_simulation_test`, `update_guide` and `compute_dice`, driven with the masks of tests/inter_eval_shapes.py, written to
tests/golden/ref_inter_eval.json (integers only).

    python tests/golden/make_inter_eval_fixtures.py     # needs the reference checkout; rewrites ref_inter_eval.json

The module imports tensorflow, cv2, skimage, GeodisTK and more at module level; the stand-ins of
make_propagation_fixtures.py are put into sys.modules first.  skimage is not installed, so `skeletonize` is replaced with a
function that raises: where the reference asks for the skeleton, the record says "fallback": true and carries no reference
click (the fallback is the project's own rule).

  singles   (pred, ref) -> click, kind
  sessions  the loop of main_eval.py:335-358 restated around the reference's own update_guide and compute_dice, with the toy
            predictor of inter_eval_shapes.disc_prediction; followed up to the first fallback round
  repeat    a session whose predictor ignores the clicks: it ends by the repeat rule"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import inter_eval_shapes as shapes  # noqa: E402
import make_propagation_fixtures as mpf  # noqa: E402

REF = mpf.REF
INTER_THRESH = 0.9
MAX_ITER = 20


class SkeletonAsked(Exception):
    pass


def _import_reference():
    mpf.STUBBED = tuple(mpf.STUBBED) + ("GeodisTK", "pandas", "matplotlib", "seaborn", "yaml", "tensorflow_core")
    sys.meta_path.insert(0, mpf._StubFinder())
    sys.path.insert(0, REF)
    from entry import main_eval

    def raises(*a, **k):
        raise SkeletonAsked()
    main_eval.skeletonize = raises
    return main_eval


def single_cases():
    """(name, shape, pred spec, ref spec)."""
    out = []
    for shape in ((40, 48), (100, 104), (140, 333)):
        h, w = shape
        obj = shapes.two_ellipses(shape)
        out.append(("object", shape, [], obj))                                            # round 0: the whole object, kind 0
        out.append(("overshoot", shape, [["+", "rect", 1, h - 1, 1, w - 1]], obj))        # a frame of false positives, kind 1
        out.append(("ring_fg", shape, [["+", "ellipse", h // 2, w // 2, h // 8, h // 8]],
                    [["+", "ellipse", h // 2, w // 2, h // 3, h // 3]]))                   # a ring of false negatives
        out.append(("ring_bg", shape, [["+", "ellipse", h // 2, w // 2, h // 3, h // 3]],
                    [["+", "ellipse", h // 2, w // 2, h // 8, h // 8]]))                   # a ring of false positives
        out.append(("ring_fg_thin", shape, [], [["+", "ring", h // 2, w // 3, h // 4, h // 4 - 2]]))
        out.append(("ring_bg_thin", shape, [["+", "ring", h // 3, w // 2, h // 5, h // 5 - 3]], []))
        out.append(("ell_fg", shape, [], [["+", "rect", 4, h - 4, 4, 9], ["+", "rect", h - 9, h - 4, 4, w - 4]]))
        out.append(("ell_bg", shape, [["+", "rect", 3, 8, 3, w - 3], ["+", "rect", 3, h - 3, w - 8, w - 3]], []))
        # the candidate lies in another component than the largest: a ring and a dot at its centre
        out.append(("ring_dot_fg", shape, [], [["+", "ring", h // 2, w // 2, h // 3, h // 3 - 3], ["+", "rect", h // 2, h // 2 + 1, w // 2, w // 2 + 1]]))
        out.append(("ring_dot_bg", shape, [["+", "ring", h // 2, w // 2, h // 3, h // 3 - 3], ["+", "rect", h // 2 - 1, h // 2 + 2, w // 2 - 1, w // 2 + 2]], []))
        # a two-way area tie: np.argmax takes the first
        out.append(("tie", shape, [], [["+", "rect", h - 9, h - 4, 3, 8], ["+", "rect", 5, 10, w - 9, w - 4]]))
        out.append(("tie_mixed", shape, [["+", "rect", 20, 24, 6, 12]], [["+", "rect", 6, 12, 20, 24]]))
        # means at exactly x.5: an even and an odd integer part, on both axes
        out.append(("half_even", shape, [], [["+", "rect", 4, 6, 10, 12]]))               # (4.5, 10.5) -> (4, 10)
        out.append(("half_odd", shape, [], [["+", "rect", 5, 7, 11, 13]]))                # (5.5, 11.5) -> (6, 12)
        out.append(("half_bg", shape, [["+", "rect", 7, 11, 21, 23]], []))                # (8.5, 21.5) -> (8, 22)
    return out


def session_cases():
    """(shape, r_fg, r_bg)."""
    return [((40, 48), 7, 4), ((40, 48), 12, 5), ((100, 104), 18, 9), ((100, 104), 30, 12), ((140, 333), 30, 14),
            ((140, 333), 55, 20)]


def run_session(me, ref, predictor, cfg):
    """main_eval.py:330-358 for one slice, around the reference's update_guide and compute_dice."""
    guide, pred, num_iter, pos = None, None, [0, 0], None
    pos_col = [[], []]
    rounds = []
    while True:
        try:
            guide, new_pos, fg, pos_col = me.update_guide(pred, ref, guide, cfg, num_iter, None, pos_col)
        except SkeletonAsked:
            return rounds, "fallback", num_iter
        if new_pos == pos:
            return rounds, "repeat", num_iter
        pos = new_pos
        pred = predictor(pos_col[0], pos_col[1])
        d = me.compute_dice(pred, ref)
        rounds.append({"click": [int(v) for v in new_pos], "kind": int(fg),
                       "counts": [int(np.count_nonzero(pred)), int(np.count_nonzero(ref)), int(np.count_nonzero(pred * ref))]})
        if d > cfg.inter_thresh:
            return rounds, "dice", num_iter
        if num_iter[0] + num_iter[1] >= cfg.max_iter:
            return rounds, "max_iter", num_iter


def main():
    me = _import_reference()
    cfg = types.SimpleNamespace(geodesic=False, stddev=5., local_enhance=True, guide_channel=2, inter_thresh=INTER_THRESH,
                                max_iter=MAX_ITER)
    singles = []
    for name, shape, pspec, rspec in single_cases():
        pred, ref = shapes.build(shape, pspec), shapes.build(shape, rspec)
        rec = {"name": name, "shape": list(shape), "pred": pspec, "ref": rspec}
        try:
            pos, fg = me.inter_simulation_test(pred, ref)
            rec.update(fallback=False, click=[int(pos[0]), int(pos[1])], kind=int(fg))
        except SkeletonAsked:
            rec.update(fallback=True)
        singles.append(rec)
    sessions = []
    for shape, r_fg, r_bg in session_cases():
        rspec = shapes.two_ellipses(shape)
        ref = shapes.build(shape, rspec)
        rounds, stop, num_iter = run_session(me, ref, lambda fg, bg: shapes.disc_prediction(shape, fg, bg, r_fg, r_bg), cfg)
        sessions.append({"shape": list(shape), "ref": rspec, "r_fg": r_fg, "r_bg": r_bg, "inter_thresh": INTER_THRESH,
                         "max_iter": MAX_ITER, "rounds": rounds, "stop": stop, "num_iter": [int(v) for v in num_iter]})
    shape = (40, 48)
    rspec = shapes.two_ellipses(shape)
    fixed = [["+", "rect", 2, 6, 2, 6]]
    rounds, stop, num_iter = run_session(me, shapes.build(shape, rspec), lambda fg, bg: shapes.build(shape, fixed), cfg)
    repeat = {"shape": list(shape), "ref": rspec, "pred": fixed, "inter_thresh": INTER_THRESH, "max_iter": MAX_ITER,
              "rounds": rounds, "stop": stop, "num_iter": [int(v) for v in num_iter]}
    with open(os.path.join(HERE, "ref_inter_eval.json"), "w") as f:
        json.dump({"singles": singles, "sessions": sessions, "repeat": repeat}, f, indent=0, sort_keys=True)
        f.write("\n")
    n_fb = sum(r["fallback"] for r in singles) + sum(s["stop"] == "fallback" for s in sessions)
    n_pin = sum(not r["fallback"] for r in singles) + sum(len(s["rounds"]) for s in sessions)
    print("pinned clicks {}, fallback clicks {}; session stops {}; repeat: {} rounds, stop {}, num_iter {}".format(
        n_pin, n_fb, [s["stop"] for s in sessions], len(rounds), stop, num_iter))


if __name__ == "__main__":
    main()
