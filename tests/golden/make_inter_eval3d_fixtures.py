"""3-D interactive-evaluation fixtures pinned on the REFERENCE ITSELF (build container only): entry/main_eval_3d.py's
`inter_simulation_test`, `update_guide` and `compute_dice`, driven with the volumes of tests/inter_eval3d_shapes.py, written to
tests/golden/ref_inter_eval3d.json (integers only).

    python tests/golden/make_inter_eval3d_fixtures.py     # needs the reference checkout; rewrites ref_inter_eval3d.json

The module imports tensorflow, cv2, skimage and more at module level; the stand-ins of make_propagation_fixtures.py are put
into sys.modules first.  The reference spells a dtype `np.bool`, an alias that numpy 2 no longer has: it is set before the
import.  skimage is not installed, so `skeletonize_3d` is replaced with a function that raises: where the reference asks for
the skeleton, the record says "fallback": true and carries no reference click (the fallback is the project's own rule,
DESIGN.md 7.3.8).

  singles   (pred, ref) -> click, kind
  sessions  the loop of main_eval_3d.py:341-384 restated around the reference's own update_guide and compute_dice, with the
            toy predictor of inter_eval3d_shapes.ball_prediction; followed up to the first fallback round
  repeat    a session whose predictor ignores the clicks: it ends by the repeat rule"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import inter_eval3d_shapes as shapes  # noqa: E402
import make_propagation_fixtures as mpf  # noqa: E402

REF = mpf.REF
INTER_THRESH = 0.9
MAX_ITER = 20
SHAPES = ((6, 20, 24), (12, 40, 48), (20, 64, 70))


class SkeletonAsked(Exception):
    pass


def _import_reference():
    if not hasattr(np, "bool"):
        np.bool = bool                                                            # main_eval_3d.py:172
    mpf.STUBBED = tuple(mpf.STUBBED) + ("GeodisTK", "pandas", "matplotlib", "seaborn", "yaml", "tensorflow_core", "skimage", "cv2",
                                        "nibabel")
    sys.meta_path.insert(0, mpf._StubFinder())
    sys.path.insert(0, REF)
    from entry import main_eval_3d

    def raises(*a, **k):
        raise SkeletonAsked()
    main_eval_3d.skeletonize_3d = raises
    return main_eval_3d


def single_cases():
    """(name, shape, pred spec, ref spec)."""
    out = []
    for shape in SHAPES:
        d, h, w = shape
        cz, cy, cx = d // 2, h // 2, w // 2
        rz = max(d // 3, 2)
        obj = shapes.two_ellipsoids(shape)
        out.append(("object", shape, [], obj))                                            # round 0: the whole object, kind 0
        out.append(("overshoot", shape, [["+", "box", 0, d, 1, h - 1, 1, w - 1]], obj))   # a shell of false positives, kind 1
        big, small = ["+", "ellipsoid", cz, cy, cx, rz, h // 3, h // 3], ["+", "ellipsoid", cz, cy, cx, 1, h // 8, h // 8]
        out.append(("shell_fg", shape, [small], [big]))                                   # a thick shell of false negatives
        out.append(("shell_bg", shape, [big], [small]))                                   # a thick shell of false positives
        out.append(("shell_fg_thin", shape, [], [["+", "shell", cz, cy, w // 3, rz, h // 4, h // 4, 1, 2]]))
        out.append(("shell_bg_thin", shape, [["+", "shell", cz, h // 3, cx, rz, h // 5, h // 5, 1, 3]], []))
        out.append(("ell_fg", shape, [], [["+", "box", 1, d - 1, 4, h - 4, 4, 9], ["+", "box", 1, d - 1, h - 9, h - 4, 4, w - 4]]))
        out.append(("ell_bg", shape, [["+", "box", 0, d - 2, 3, 8, 3, w - 3], ["+", "box", 0, d - 2, 3, h - 3, w - 8, w - 3]], []))
        # the candidate lies in another component than the largest: a shell and a dot at its centre
        shell = ["+", "shell", cz, cy, cx, rz, h // 3, h // 3, 1, 2]
        out.append(("shell_dot_fg", shape, [], [shell, ["+", "box", cz, cz + 1, cy, cy + 1, cx, cx + 1]]))
        out.append(("shell_dot_bg", shape, [shell, ["+", "box", cz, cz + 1, cy - 1, cy + 2, cx - 1, cx + 2]], []))
        # a two-way size tie: np.argmax takes the first
        out.append(("tie", shape, [], [["+", "box", d - 3, d - 1, h - 9, h - 4, 3, 8], ["+", "box", 1, 3, 5, 10, w - 9, w - 4]]))
        out.append(("tie_mixed", shape, [["+", "box", 3, 5, 14, 18, 6, 12]], [["+", "box", 1, 3, 6, 12, 14, 18]]))
        # means at exactly x.5 on every axis: an even and an odd integer part
        out.append(("half_even", shape, [], [["+", "box", 2, 4, 4, 6, 10, 12]]))          # (2.5, 4.5, 10.5) -> (2, 4, 10)
        out.append(("half_odd", shape, [], [["+", "box", 1, 3, 5, 7, 11, 13]]))           # (1.5, 5.5, 11.5) -> (2, 6, 12)
        out.append(("half_bg", shape, [["+", "box", 3, 5, 7, 11, 21, 23]], []))           # (3.5, 8.5, 21.5) -> (4, 8, 22)
        # compact cases of both kinds beside the object: the reference places these itself
        out.append(("blob_bg", shape, [["+", "ellipsoid", cz, cy, cx, 2, h // 5, w // 6]], []))
        out.append(("slab_fg", shape, [["+", "box", 0, d, 0, h, 0, cx]], [["+", "box", 0, d, 0, h, 0, cx + 3]]))
    return out


def session_cases():
    """(shape, r_fg, r_bg): radii (z, in-plane)."""
    return [((6, 20, 24), (1, 3), (1, 2)), ((6, 20, 24), (2, 6), (1, 3)), ((12, 40, 48), (2, 7), (1, 4)),
            ((12, 40, 48), (4, 12), (2, 5)), ((20, 64, 70), (4, 12), (2, 6)), ((20, 64, 70), (7, 20), (3, 8))]


def run_session(me, ref, predictor, cfg):
    """main_eval_3d.py:335-384 for one case, around the reference's update_guide and compute_dice."""
    guide, pred, num_iter, pos = None, None, [0, 0], None
    pos_col = [[], []]
    rounds = []
    ref = ref.astype(bool)                                                        # :321 label_bool
    while True:
        try:
            guide, new_pos, fg, pos_col = me.update_guide(pred, ref, guide, cfg, num_iter, pos_col)
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
    cfg = types.SimpleNamespace(stddev=[1., 3., 3.], local_enhance=True, guide_channel=2, inter_thresh=INTER_THRESH,
                                max_iter=MAX_ITER)
    singles = []
    for name, shape, pspec, rspec in single_cases():
        pred, ref = shapes.build(shape, pspec), shapes.build(shape, rspec).astype(bool)
        rec = {"name": name, "shape": list(shape), "pred": pspec, "ref": rspec}
        try:
            pos, fg = me.inter_simulation_test(pred, ref)
            rec.update(fallback=False, click=[int(v) for v in pos], kind=int(fg))
        except SkeletonAsked:
            rec.update(fallback=True)
        singles.append(rec)
    sessions = []
    for shape, r_fg, r_bg in session_cases():
        rspec = shapes.two_ellipsoids(shape)
        ref = shapes.build(shape, rspec)
        rounds, stop, num_iter = run_session(me, ref, lambda fg, bg: shapes.ball_prediction(shape, fg, bg, r_fg, r_bg), cfg)
        sessions.append({"shape": list(shape), "ref": rspec, "r_fg": list(r_fg), "r_bg": list(r_bg), "inter_thresh": INTER_THRESH,
                         "max_iter": MAX_ITER, "rounds": rounds, "stop": stop, "num_iter": [int(v) for v in num_iter]})
    shape = SHAPES[0]
    rspec = shapes.two_ellipsoids(shape)
    fixed = [["+", "box", 0, 2, 1, 4, 1, 4]]
    rounds, stop, num_iter = run_session(me, shapes.build(shape, rspec), lambda fg, bg: shapes.build(shape, fixed), cfg)
    repeat = {"shape": list(shape), "ref": rspec, "pred": fixed, "inter_thresh": INTER_THRESH, "max_iter": MAX_ITER,
              "rounds": rounds, "stop": stop, "num_iter": [int(v) for v in num_iter]}
    with open(os.path.join(HERE, "ref_inter_eval3d.json"), "w") as f:
        json.dump({"singles": singles, "sessions": sessions, "repeat": repeat}, f, indent=0, sort_keys=True)
        f.write("\n")
    n_fb = sum(r["fallback"] for r in singles) + sum(s["stop"] == "fallback" for s in sessions)
    n_pin = sum(not r["fallback"] for r in singles) + sum(len(s["rounds"]) for s in sessions)
    print("pinned clicks {}, fallback clicks {}; session stops {}; repeat: {} rounds, stop {}, num_iter {}".format(
        n_pin, n_fb, [s["stop"] for s in sessions], len(rounds), stop, num_iter))
    for r in singles:
        print(r["name"], r["shape"], "fallback" if r["fallback"] else (r["click"], r["kind"]))
    for s in sessions:
        print(s["shape"], s["r_fg"], s["r_bg"], [(q["click"], q["kind"]) for q in s["rounds"]], s["stop"])


if __name__ == "__main__":
    main()
