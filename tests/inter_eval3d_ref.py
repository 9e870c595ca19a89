"""Host restatement of the 3-D interactive evaluator's click step and session loop, written with
scipy.ndimage.label and distance_transform_cdt("taxicab").  It cites the reference's entry/main_eval_3d.py; the records of
tests/golden/ref_inter_eval3d.json hold it to the reference (tests/test_inter_eval3d_host.py), and the GPU tests hold the
kernel to it where no record exists (the fallback is the project's own rule)."""
import numpy as np
import scipy.ndimage as ndi

CAP = 255
TAB_COLS = 20


def round_half_even_div(s, a):
    """s / a rounded half to even, in integers (np.mean(...).round(0) of exact integers)."""
    q, r = divmod(int(s), int(a))
    if 2 * r > a or (2 * r == a and q % 2 == 1):
        q += 1
    return q


def counts(pred, ref):
    """(n_pred, n_ref, n_inter) of two binary volumes."""
    p, r = pred.astype(bool), ref.astype(bool)
    return int(p.sum()), int(r.sum()), int((p & r).sum())


def dice(n_pred, n_ref, n_inter):
    """compute_dice (main_eval_3d.py:210-213) from the integer counts, float64."""
    return (2 * n_inter + 1e-8) / (n_pred + n_ref + 1e-8)


def city_block(err, cap=CAP):
    """Distance of every voxel to the nearest non-error voxel, the volume's border counting as one, capped."""
    return np.minimum(ndi.distance_transform_cdt(np.pad(err, 1), metric="taxicab")[1:-1, 1:-1, 1:-1], cap)


def click(pred, ref, cap=CAP):
    """inter_simulation_test (main_eval_3d.py:152-185) with the project's fallback.  Returns a dict: counts, n_comp, area,
    root, cand, click, kind, fallback, empty."""
    p, r = pred.astype(bool), ref.astype(bool)
    err = p ^ r
    d, h, w = err.shape
    none = (-1, -1, -1)
    out = {"counts": counts(p, r), "n_comp": 0, "area": 0, "root": -1, "cand": none, "click": none, "kind": -1,
           "fallback": False, "empty": not err.any()}
    if out["empty"]:
        return out
    res, n_obj = ndi.label(err, ndi.generate_binary_structure(3, 1))
    sizes = np.bincount(res.ravel())
    max_i = int(np.argmax(sizes[1:])) + 1                      # the first maximum: the component met first in (z, y, x) order
    zs, ys, xs = np.nonzero(res == max_i)
    cand = tuple(round_half_even_div(s.sum(), s.size) for s in (zs, ys, xs))
    out.update(n_comp=int(n_obj), area=int(zs.size), root=int((zs[0] * h + ys[0]) * w + xs[0]), cand=cand)
    pos = cand
    if not err[cand]:
        # the project's rule in place of skeletonize_3d: the component's voxel farthest (city block, capped) from the nearest
        # non-error voxel, the border counting as one; ties: nearer to the candidate, then the smaller linear index
        dist = city_block(err, cap)[zs, ys, xs].astype(np.int64)
        d2 = (zs - cand[0]) ** 2 + (ys - cand[1]) ** 2 + (xs - cand[2]) ** 2
        first = np.lexsort(((zs * h + ys) * w + xs, d2, -dist))[0]
        pos = (int(zs[first]), int(ys[first]), int(xs[first]))
        out["fallback"] = True
    out["click"] = tuple(int(v) for v in pos)
    out["kind"] = 0 if r[pos] else 1
    return out


def table_row(pred, ref, prev=None, have=(0, 0), k=64, cap=CAP):
    """The int32 row unetk_inter_click3d writes for a case inside the store (include/unetk.h), and the click it appends:
    (row, kind or -1, click or None, appended)."""
    c = click(pred, ref, cap)
    row = np.zeros(TAB_COLS, dtype=np.int32)
    row[5:13] = -1
    row[0:3] = c["counts"]
    row[17] = 1
    if c["empty"]:
        row[15] = 1
        return row, -1, None, False
    row[3], row[4], row[5] = c["n_comp"], c["area"], c["root"]
    row[6:9], row[9:12], row[12] = c["cand"], c["click"], c["kind"]
    row[13] = int(c["fallback"])
    row[14] = int(prev is not None and tuple(prev) == c["click"])
    appended = min(max(int(have[c["kind"]]), 0), k) < k
    row[16] = int(appended)
    return row, c["kind"], c["click"], appended


def session(ref, predictor, inter_thresh, max_iter, on_round=None, cap=CAP):
    """The loop of main_eval_3d.py:341-384 for one case: predictor(fg_clicks, bg_clicks) -> prediction volume.  Returns
    (rounds, stop, num_iter): rounds = [(click, kind, fallback, counts after the forward)], stop in {"repeat", "dice",
    "max_iter", "empty"}."""
    pred = np.zeros_like(ref, dtype=np.uint8)
    lists, num_iter, pos, rounds = ([], []), [0, 0], None, []
    while True:
        c = click(pred, ref, cap)
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
