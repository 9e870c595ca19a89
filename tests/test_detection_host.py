"""Host: per-lesion detection -- the matching rule on component tables (array_kits.match_components), the
two array_kits functions against the restatement in detection_ref.py, the inf rule of the metrics, the evaluator's flags,
and the refusals of unetk_component_overlaps that return before anything is launched."""
import argparse
import ctypes

import numpy as np
import pytest

import detection_ref as dref

E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
SEED, N_PAIRS, SHAPE = 5, 50, (8, 24, 24)


def _match(res_sizes, ref_sizes, pairs, thresh=0.5):
    from boxsegliver_amd.utils import array_kits
    return array_kits.match_components(np.array(res_sizes), np.array(ref_sizes), np.array(pairs).reshape(-1, 3), thresh)


# ------------------------------------------------------------------------------------------------- the matching rule
def test_single_candidate_accepted_with_the_dice_score():
    m = _match([10], [10], [(1, 1, 6)])
    assert m == {1: [1, 2 * 6 / 20.0]}
    assert 6 / 14.0 < 0.5 <= 0.6                       # its IoU (6 / 14) would have failed the threshold: the score is Dice
    assert type(m[1][0]) is int and type(m[1][1]) is float


def test_single_candidate_below_threshold():
    assert _match([10], [10], [(1, 1, 4)]) == {}       # 8 / 20
    assert _match([10], [10], [(1, 1, 5)]) == {1: [1, 0.5]}          # >= : the threshold itself passes
    assert _match([10], [10], [(1, 1, 5)], thresh=0.51) == {}
    assert _match([3, 4], [5], []) == {}


def test_single_candidate_already_used_stays_unmatched():
    # result 1 (20 voxels) covers reference 1 and reference 2 (10 each); reference 2 would score 2 * 10 / 30 >= 0.5 as well
    m = _match([20], [10, 10], [(1, 1, 10), (2, 1, 10)])
    assert m == {1: [1, 2 * 10 / 30.0]}
    # ... and it is not tried again later, even though a waiting object frees nothing it could use
    m = _match([20, 10], [10, 10, 10], [(1, 1, 10), (2, 1, 10), (3, 1, 1), (3, 2, 9)])
    assert m == {1: [1, 2 * 10 / 30.0], 3: [2, 2 * 9 / 20.0]}


def test_several_candidates_largest_overlap_fails_and_the_next_passes():
    # reference 1 (10 voxels): 6 of them in result 1, a 100-voxel object (12 / 110), 4 in result 2 of 4 voxels (8 / 14)
    m = _match([100, 4], [10], [(1, 1, 6), (1, 2, 4)])
    assert m == {1: [2, 8 / 14.0]}
    assert _match([100, 4], [10], [(1, 1, 6), (1, 2, 4)], thresh=0.6) == {}


def test_set_size_decides_who_gets_a_contested_result_object():
    # reference 1 overlaps results {1, 2, 3}, reference 2 overlaps {1, 2}: the smaller set goes first and takes result 1,
    # which reference 1 would have taken had the ids decided; reference 1 is left with result 2
    res = [10, 10, 10]
    ref = [12, 10]
    pairs = [(1, 1, 6), (1, 2, 5), (1, 3, 1), (2, 1, 4), (2, 2, 3)]
    m = _match(res, ref, pairs, thresh=0.3)
    assert m == {2: [1, 2 * 4 / 20.0], 1: [2, 2 * 5 / 22.0]}
    assert list(m) == [2, 1]                           # the order they were decided in
    # a used candidate shrinks a set before the sort: reference 3's single candidate takes result 3 first, so reference 1's
    # set {2, 3, 4} shrinks to two and ties with reference 2's {1, 2}; the stable sort keeps the id order and
    # reference 1 takes the contested result 2
    m = _match([10, 10, 10, 10], [10, 10, 10],
               [(1, 2, 5), (1, 3, 4), (1, 4, 1), (2, 1, 1), (2, 2, 6), (3, 3, 6)], thresh=0.3)
    assert m == {3: [3, 0.6], 1: [2, 0.5]}             # reference 2 is left with result 1: 2 / 20 is below 0.3


def test_both_tie_rules():
    # equal overlaps inside one set: the lowest result id is tried first
    m = _match([5, 5], [10], [(1, 1, 5), (1, 2, 5)], thresh=0.1)
    assert m == {1: [1, 10 / 15.0]}
    m = _match([5, 5], [10], [(1, 2, 5), (1, 1, 5)], thresh=0.1)       # whatever order the rows come in
    assert m == {1: [1, 10 / 15.0]}
    # equal set sizes: the stable sort keeps the reference ids in order, so reference 1 picks before reference 2
    m = _match([8, 8], [8, 8], [(1, 1, 4), (1, 2, 4), (2, 1, 4), (2, 2, 4)])
    assert m == {1: [1, 0.5], 2: [2, 0.5]}


# ------------------------------------------------------------------------------------------------- against the restatement
def _random_pairs():
    rng = np.random.default_rng(SEED)
    for t in range(N_PAIRS):
        a = dref.blob(rng, SHAPE, rng.uniform(0.03, 0.09), sigma=rng.uniform(1.4, 2.0))
        b = dref.blob(rng, SHAPE, rng.uniform(0.03, 0.09), sigma=rng.uniform(1.4, 2.0))
        if t % 3 != 2:                                 # correlated pairs (a shifted copy, cut and joined by other blobs): objects that match
            shift = tuple(int(s) for s in rng.integers(-1, 2, 3))
            b = np.roll(a, shift, (0, 1, 2)) ^ b
        yield a, b


def test_array_kits_agree_with_the_restatement_on_random_volumes():
    from boxsegliver_amd.utils import array_kits
    from boxsegliver_amd import loss_metrics
    looped = matched = 0
    for t, (a, b) in enumerate(_random_pairs()):
        stats = {}
        thresh = (0.5, 0.3, 0.1)[t % 3]
        n_res, n_ref, want = dref.correspondences(a, b, thresh, stats)
        assert 3 <= n_res <= 30 and 3 <= n_ref <= 30, (t, n_res, n_ref)
        looped += stats["waiting"] > 0
        matched += len(want) > 0
        lres, lref, res_sizes, ref_sizes, pairs = dref.label_tables(a, b)
        got = array_kits.match_components(res_sizes, ref_sizes, pairs, thresh)
        assert got == want and list(got) == list(want), t
        out = array_kits.distinct_binary_object_correspondences(a, b, thresh)
        np.testing.assert_array_equal(out[0], lres)
        np.testing.assert_array_equal(out[1], lref)
        assert out[2:4] == (n_res, n_ref) and out[4] == want and list(out[4]) == list(want), t
        assert loss_metrics.tumor_detection_metrics(a.astype(np.uint8), b.astype(np.uint8), thresh) == \
            dref.detection_metrics(a, b, thresh), t
    assert looped >= 10, looped                        # the several-candidates loop is reached
    assert matched >= 10, matched


def test_connectivity_other_than_faces_is_refused():
    from boxsegliver_amd.utils import array_kits
    from boxsegliver_amd import loss_metrics
    a = np.ones((2, 2, 2), bool)
    for c in (2, 3):
        with pytest.raises(ValueError, match="connectivity"):
            array_kits.distinct_binary_object_correspondences(a, a, 0.5, c)
        with pytest.raises(ValueError, match="connectivity"):
            loss_metrics.tumor_detection_metrics(a, a, connectivity=c)


# ------------------------------------------------------------------------------------------------- metrics
def test_precision_and_recall_are_inf_over_a_zero_denominator():
    from boxsegliver_amd import loss_metrics
    empty, one = np.zeros((3, 4, 5), np.uint8), np.zeros((3, 4, 5), np.uint8)
    one[1, 1:3, 2] = 1
    r = loss_metrics.tumor_detection_metrics(empty, one)
    assert r == {"tp": 0, "fp": 0, "pos": 1, "precision": np.inf, "recall": 0.0}
    r = loss_metrics.tumor_detection_metrics(one, empty)
    assert r == {"tp": 0, "fp": 1, "pos": 0, "precision": 0.0, "recall": np.inf}
    r = loss_metrics.tumor_detection_metrics(empty, empty)
    assert r == {"tp": 0, "fp": 0, "pos": 0, "precision": np.inf, "recall": np.inf}
    r = loss_metrics.tumor_detection_metrics(one, one)
    assert r == {"tp": 1, "fp": 0, "pos": 1, "precision": 1.0, "recall": 1.0}
    assert list(r) == ["tp", "fp", "pos", "precision", "recall"]
    assert loss_metrics.detection_scores(3, 4, 6) == {"tp": 3, "fp": 1, "pos": 6, "precision": 0.75, "recall": 0.5}


# ------------------------------------------------------------------------------------------------- flags
ARGV = "--mode eval --tag t --model UNet --classes Liver Tumor --evaluator Volume".split()


def test_flags_parse_and_default_to_off():
    from boxsegliver_amd.entry import main as entry
    for guided, subs in ((False, ("liver", "only_liver", "liver_3d", "nf")), (True, ("liver", "nf"))):
        for sub in subs:
            args = entry.get_arguments([sub] + ARGV, guided=guided)[0]
            assert args.eval_detection is False and args.detection_thresh == 0.5, sub
            args = entry.get_arguments([sub] + ARGV + "--eval_detection --detection_thresh 0.25".split(), guided=guided)[0]
            assert args.eval_detection is True and args.detection_thresh == 0.25, sub


class _FakeModel(object):
    def __init__(self, classes):
        self.classes = ["Background"] + list(classes)


def _evaluator(classes, **over):
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    args = argparse.Namespace(eval_mirror=False, random_flip=0, metrics_eval=["Dice"], use_global_dice=False, pred_type="pred",
                              mode="eval", im_height=16, im_width=16, eval_num=-1, classes=list(classes))
    for k, v in over.items():
        setattr(args, k, v)
    return ev.EvaluateVolume(estimator=None, model_dir=".", params={"args": args, "model_instances": [_FakeModel(classes)]})


def test_detection_needs_a_tumor_class():
    with pytest.raises(ValueError, match="Tumor"):
        _evaluator(["Liver"], eval_detection=True)
    assert _evaluator(["Liver"]).eval_detection is False
    assert _evaluator(["Liver"], eval_detection=False).eval_detection is False
    e = _evaluator(["Liver", "Tumor"], eval_detection=True, detection_thresh=0.3)
    assert e.eval_detection is True and e.detection_thresh == 0.3


def test_summed_counts_give_the_run_precision_and_recall():
    from collections import defaultdict
    e = _evaluator(["Liver", "Tumor"], eval_detection=True)
    acc = defaultdict(int)
    e._add_detection(acc, {"tp": 2, "fp": 1, "pos": 4, "precision": 2 / 3, "recall": 0.5})
    e._add_detection(acc, {"tp": 1, "fp": 0, "pos": 1, "precision": 1.0, "recall": 1.0})
    assert dict(acc) == {"Tumor_det_tp": 3, "Tumor_det_fp": 1, "Tumor_det_pos": 5}
    assert e._detection_results(acc) == {"Tumor/DetTP": 3, "Tumor/DetFP": 1, "Tumor/DetPos": 5, "Tumor/Precision": 0.75,
                                         "Tumor/Recall": 0.6}
    r = e._detection_results(defaultdict(int))
    assert r["Tumor/Precision"] == np.inf and r["Tumor/Recall"] == np.inf and r["Tumor/DetPos"] == 0


# ------------------------------------------------------------------------------------------------- C ABI without a device
def test_component_overlaps_refusals_return_before_any_launch():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_component_overlaps_ws_bytes", "unetk_component_overlaps"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.unetk_abi_version() == _abi.ABI_VERSION == 10                   # an additive change
    d, h, w = 7, 13, 17
    n = d * h * w
    nbytes = lib.unetk_component_overlaps_ws_bytes(d, h, w, 16, 32)
    assert nbytes >= 16 * n + 16 * 32
    p = ctypes.c_void_p(1 << 20)                                               # never dereferenced: every call below is refused
    call = lib.unetk_component_overlaps
    assert call(None, p, d, h, w, 16, 32, p, p, nbytes, None) == E_BADARG      # NULL pointers
    assert call(p, None, d, h, w, 16, 32, p, p, nbytes, None) == E_BADARG
    assert call(p, p, d, h, w, 16, 32, None, p, nbytes, None) == E_BADARG
    assert call(p, p, d, h, w, 16, 32, p, None, nbytes, None) == E_BADARG
    assert call(p, p, d, h, w, 16, 32, ctypes.c_void_p((1 << 20) + 2), p, nbytes, None) == E_BADARG     # misaligned table
    assert call(p, p, d, h, w, 16, 32, p, ctypes.c_void_p((1 << 20) + 8), nbytes, None) == E_BADARG     # misaligned workspace
    for caps in ((0, 32), (16, 0), (-1, 32), (16, -5)):                        # caps <= 0
        assert call(p, p, d, h, w, caps[0], caps[1], p, p, 1 << 30, None) == E_BADARG, caps
        assert lib.unetk_component_overlaps_ws_bytes(d, h, w, *caps) == 0, caps
    assert call(p, p, 0, h, w, 16, 32, p, p, nbytes, None) == E_BADARG
    assert call(p, p, d, h, w, 16, 32, p, p, nbytes - 1, None) == E_WORKSPACE  # a short workspace
    assert call(p, p, d, h, w, 16, 32, p, p, 0, None) == E_WORKSPACE
    for dims in ((2048, 1024, 1024), (1291, 1291, 1291), (1 << 16, 1 << 15, 1)):      # D * H * W >= 2^31
        assert call(p, p, dims[0], dims[1], dims[2], 16, 32, p, p, 1 << 40, None) == E_UNSUPPORTED, dims
        assert lib.unetk_component_overlaps_ws_bytes(dims[0], dims[1], dims[2], 16, 32) == 0, dims
    assert lib.unetk_component_overlaps_ws_bytes(1, 1, (1 << 31) - 1, 16, 32) > 0
    assert lib.unetk_component_overlaps_ws_bytes(450, 512, 512, 65536, 262144) < 2 << 30
