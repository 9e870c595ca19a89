"""Host restatement of the interactive evaluator's click step and session loop, written with
scipy.ndimage.label and distance_transform_cdt("taxicab").  It cites the reference's entry/main_eval.py; the records of
tests/golden/ref_inter_eval.json hold it to the reference (tests/test_inter_eval_host.py), and the GPU tests hold the kernel
to it where no record exists (the fallback is the project's own rule)."""
import numpy as np
import scipy.ndimage as ndi

CAP = 255


def round_half_even_div(s, a):
    """s / a rounded half to even, in integers (np.mean(...).round(0) of exact integers)."""
    q, r = divmod(int(s), int(a))
    if 2 * r > a or (2 * r == a and q % 2 == 1):
        q += 1
    return q


def counts(pred, ref):
    """(n_pred, n_ref, n_inter) of two binary masks."""
    p, r = pred.astype(bool), ref.astype(bool)
    return int(p.sum()), int(r.sum()), int((p & r).sum())


def dice(n_pred, n_ref, n_inter):
    """compute_dice (main_eval.py:225-228) from the integer counts, float64."""
    return (2 * n_inter + 1e-8) / (n_pred + n_ref + 1e-8)


def click(pred, ref):
    """inter_simulation_test (main_eval.py:149-183) with the project's fallback.  Returns a dict: counts, n_comp, area, root,
    cand, click, kind, fallback, empty."""
    p, r = pred.astype(bool), ref.astype(bool)
    err = p ^ r
    h, w = err.shape
    out = {"counts": counts(p, r), "n_comp": 0, "area": 0, "root": -1, "cand": (-1, -1), "click": (-1, -1), "kind": -1,
           "fallback": False, "empty": not err.any()}
    if out["empty"]:
        return out
    res, n_obj = ndi.label(err, ndi.generate_binary_structure(2, 1))
    sizes = np.bincount(res.ravel())
    max_i = int(np.argmax(sizes[1:])) + 1                      # the first maximum: the component met first in row-major order
    comp = res == max_i
    ys, xs = np.nonzero(comp)
    cy, cx = round_half_even_div(ys.sum(), ys.size), round_half_even_div(xs.sum(), xs.size)
    out.update(n_comp=int(n_obj), area=int(ys.size), root=int(ys[0] * w + xs[0]), cand=(cy, cx))
    y, x = cy, cx
    if not err[cy, cx]:
        # the project's rule in place of skeletonize: the component's pixel farthest (city block, capped) from the nearest
        # non-error pixel, the border counting as one; ties: nearer to the candidate, then the smaller linear index
        dist = np.minimum(ndi.distance_transform_cdt(np.pad(err, 1), metric="taxicab")[1:-1, 1:-1], CAP)
        d = dist[ys, xs].astype(np.int64)
        d2 = (ys - cy) ** 2 + (xs - cx) ** 2
        order = np.lexsort((ys * w + xs, d2, -d))
        y, x = int(ys[order[0]]), int(xs[order[0]])
        out["fallback"] = True
    out["click"] = (int(y), int(x))
    out["kind"] = 0 if r[y, x] else 1
    return out


def session(ref, predictor, inter_thresh, max_iter, on_round=None):
    """The loop of main_eval.py:335-358 for one slice: predictor(fg_clicks, bg_clicks) -> prediction at the slice's
    resolution.  Returns (rounds, stop, num_iter): rounds = [(click, kind, fallback, counts after the forward)], stop in
    {"repeat", "dice", "max_iter", "empty"}."""
    pred = np.zeros_like(ref, dtype=np.uint8)
    lists, num_iter, pos, rounds = ([], []), [0, 0], None, []
    while True:
        c = click(pred, ref)
        if c["empty"]:
            return rounds, "empty", num_iter
        lists[c["kind"]].append(c["click"])
        num_iter[c["kind"]] += 1
        if c["click"] == pos:
            return rounds, "repeat", num_iter
        pos = c["click"]
        pred = predictor(lists[0], lists[1])
        n = counts(pred, ref)
        rounds.append((c["click"], c["kind"], c["fallback"], n))
        if on_round is not None:
            on_round(c, pred)
        if dice(*n) > inter_thresh:
            return rounds, "dice", num_iter
        if num_iter[0] + num_iter[1] >= max_iter:
            return rounds, "max_iter", num_iter
