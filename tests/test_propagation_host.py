"""Host: the spatial-guide propagation of the guided volume evaluation (boxsegliver_amd/data/propagate.py) against the
reference's own EvalImage3DLoader and simulate_user_prior (tests/golden/ref_propagation.npz, made by
tests/golden/make_propagation_fixtures.py), the numpy restatements of unetk_guide_components / unetk_guide_render, the prior
file, the --eval_no_sp slabs and the entry's routing."""
import argparse
import json
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

from boxsegliver_amd.data import extract, propagate
from boxsegliver_amd.utils import array_kits

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_propagation.npz")
PSHAPE = (48, 48)
MIN_STD, DISCOUNT = 2.0, 0.85


def _fixture():
    f = np.load(FIXTURE)
    return {k: f[k] for k in f.files}


def test_prior_file_equals_the_references_on_the_meta_excerpt():
    excerpt = json.load(open(os.path.join(HERE, "golden", "ref_meta_excerpt.json")))["cases"]
    want = json.loads(str(_fixture()["prior_json"]))
    got = json.loads(json.dumps(extract.simulate_user_prior(excerpt)))
    assert got == want
    assert sum(len(v) for case in want.values() for v in case.values()) > 0


def test_prior_command_writes_prior_json(tmp_path):
    excerpt = json.load(open(os.path.join(HERE, "golden", "ref_meta_excerpt.json")))["cases"]
    (tmp_path / "meta.json").write_text(json.dumps(excerpt))
    extract.main(["prior", str(tmp_path)])
    assert json.loads((tmp_path / "prior.json").read_text()) == json.loads(str(_fixture()["prior_json"]))
    assert propagate.load_prior(tmp_path) == json.loads((tmp_path / "prior.json").read_text())
    with pytest.raises(FileNotFoundError, match="extract prior"):
        propagate.load_prior(tmp_path / "nowhere")
    assert propagate.load_prior(tmp_path / "nowhere", real_sp=str(tmp_path / "prior.json"))


def _objects_of(info):
    return [{"z": list(o["z"]), "center": [int(v) for v in o["center"]], "stddev": [float(v) for v in o["stddev"]]}
            for o in info]


def test_state_machine_replays_the_reference_step_by_step():
    fx = _fixture()
    prior = json.loads(str(fx["scenario_prior"]))
    cases = {c["pid"]: c for c in json.loads(str(fx["cases"]))}
    steps = json.loads(str(fx["steps"]))
    guides = dict(zip(fx["guide_steps"].tolist(), fx["guides"]))
    state = propagate.Propagation(prior, MIN_STD, DISCOUNT, PSHAPE)
    seen = {"low": 0, "ended": 0, "kept": 0, "ascent": 0, "carry": 0, "error": 0}
    for i, (step, mask) in enumerate(zip(steps, fx["masks"])):
        case = cases[step["pid"]]
        objects = state.start_slice(step["pid"], step["sid"], case["bbox"], case["cshape"])
        assert _objects_of(state.curr_info) == _objects_of(step["curr"]), i
        guide = propagate.render_numpy(objects, PSHAPE, DISCOUNT)
        if i in guides:
            np.testing.assert_array_equal(guide, guides[i])
        comps = propagate.components_numpy(mask, guide)
        if step["error"]:
            with pytest.raises(ValueError, match="Can not find corresponding guide!"):
                state.finish_slice(step["sid"], comps, guide)
            seen["error"] += 1
            break
        before = _objects_of(state.last_info)
        decisions = state.finish_slice(step["sid"], comps, guide)
        assert _objects_of(state.last_info) == _objects_of(step["last"]), i
        if not comps and before:
            assert _objects_of(state.last_info) == before
            seen["carry"] += 1
        for comp, d in zip(comps, decisions):
            key = d if isinstance(d, str) else "kept"
            seen[key] += 1
            if key == "kept" and tuple(comp.peak) not in [tuple(o["center"]) for o in state.curr_info]:
                seen["ascent"] += 1
    assert all(v > 0 for v in seen.values()), seen
    # carry-over between the sweeps and between the cases
    up_end = [s for s in steps if s["pid"] == 7 and s["direction"] == "Forward"][-1]
    assert up_end["last"] and _objects_of(up_end["last"])[0] in _objects_of(steps[steps.index(up_end) + 1]["curr"])
    first_b = [s for s in steps if s["pid"] == 8][0]
    assert first_b["curr"] and all(o["z"] == [100, 111] for o in first_b["curr"])


def test_components_numpy_rules():
    """4-connectivity (corner contacts split), raster order of the first pixel, the first maximum as the peak, and the
    moments of array_kits.compute_robust_moments."""
    rng = np.random.default_rng(3)
    mask = (rng.random((40, 52)) < 0.3).astype(np.uint8)
    mask[0:3, 0:3] = 1
    mask[3, 3] = 1                                   # corner contact only
    guide = rng.random((40, 52)).astype(np.float32)
    guide[10:14, 10:14] = np.float32(2.0)             # ties on the peak
    comps = propagate.components_numpy(mask, guide)
    lab, n = ndi.label(mask, ndi.generate_binary_structure(2, 1))
    assert len(comps) == n and [c.root for c in comps] == sorted(c.root for c in comps)
    for k, c in enumerate(comps):
        obj = lab == k + 1
        assert c.area == obj.sum() and lab.flat[c.root] == k + 1 and np.flatnonzero(obj)[0] == c.root
        vals = np.where(obj, guide, -1)
        assert c.peak == np.unravel_index(int(np.argmax(vals)), vals.shape)
        ctr, std = array_kits.compute_robust_moments(obj, indexing="ij", min_std=0.)
        np.testing.assert_array_equal(c.center, ctr)
        np.testing.assert_array_equal(c.stddev, std.astype(np.float32))
    assert lab[3, 3] != lab[2, 2]


def test_parse_table_round_trip_and_overflow():
    rows = np.zeros((2, 12), np.int32)
    rows[:, :7] = [[5, 3, 0, 5, 0, 7, 6], [60, 1, 1, 10, 1, 10, 60]]
    f = rows.view(np.float32)
    f[:, 7:] = [[0.7, 0.0, 6.0, 0.0, 1.4826], [0.9, 1.0, 10.0, 0.0, 0.0]]
    table = np.concatenate([np.array([2, 0, 0, 0], np.int32), rows.ravel()])
    comps, n_low = propagate.parse_table(table, 50)
    assert n_low == 0 and [c.peak for c in comps] == [(0, 6), (1, 10)] and comps[1].box == (1, 10, 1, 10)
    assert comps[0].peak_value == np.float32(0.7) and comps[0].stddev[1] == np.float32(1.4826)
    f[0, 7] = 0.6                                                 # below 0.15 + 0.5: only counted
    table = np.concatenate([np.array([2, 0, 0, 0], np.int32), rows.ravel()])
    kept, n_low = propagate.parse_table(table, 50, skip_low=True)
    assert n_low == 1 and [c.root for c in kept] == [60]
    table[1] = 1
    with pytest.raises(RuntimeError, match="capacity"):
        propagate.parse_table(table, 50)


def test_low_components_left_out_still_clear_last_info():
    """A slice whose only tumours are below the threshold clears last_info like the reference (its mask is not empty),
    whether the low components are listed or only counted; an empty slice keeps it."""
    state = propagate.Propagation({"1": {}}, MIN_STD, DISCOUNT, PSHAPE)
    carried = [{"z": [0, 9], "center": [5, 5], "stddev": [3.0, 3.0]}]
    state.last_info = list(carried)
    state.start_slice(1, 3, [0, 0, 0, 47, 47, 8], [11, 48, 48])
    assert state.finish_slice(3, [], None, n_low=0) == [] and state.last_info == carried
    assert state.finish_slice(3, [], None, n_low=2) == [] and state.last_info == []


def test_render_numpy_formula():
    obj = np.array([[10, 12, 2.5, 4.0], [30, 30, 3.0, 3.0]], np.float32)
    g = propagate.render_numpy(obj, (40, 44), 0.85)
    y, x = np.mgrid[0:40, 0:44]
    want = np.maximum(*(np.exp(-((y - o[0]) ** 2 / (2 * o[2] ** 2) + (x - o[1]) ** 2 / (2 * o[3] ** 2))) for o in obj))
    np.testing.assert_allclose(g, want * 0.85 / 2 + 0.5, atol=1e-6)
    assert g.dtype == np.float32
    assert np.all(propagate.render_numpy(np.zeros((0, 4)), (5, 6), 0.85) == np.float32(0.5))


def test_ascent_line_and_wu_line():
    xs, ys, fwd = array_kits.xiaolinwu_line(0, 0, 5, 2)
    assert fwd and xs == [0, 1, 2, 3, 4, 5] and ys[0] == 0 and ys[-1] == 2
    xs, ys, fwd = array_kits.xiaolinwu_line(2, 7, 0, 0)          # steep, backward
    assert not fwd and ys == list(range(0, 8)) and xs[0] == 0 and xs[-1] == 2
    with pytest.raises(ValueError):
        array_kits.xiaolinwu_line(1, 1, 1, 1)
    img = propagate.render_numpy(np.array([[20, 20, 4, 4]], np.float32), (40, 40), 0.85)
    assert propagate.ascent_line(img, 30, 35, 20, 20) and propagate.ascent_line(img, 5, 2, 20, 20)
    img[27, 24] = 0.0                                           # a dip on the way
    assert not propagate.ascent_line(img, 30, 35, 20, 20)


def test_sweeps_order():
    assert propagate.sweeps([6, 10, 10], 1, 1) == [("Forward", i) for i in (1, 2, 3, 4)] + \
        [("Backward", i) for i in (4, 3, 2, 1)]


@pytest.mark.parametrize("extra,match", [("--mode infer", "infer"), ("--mode infer --eval_no_sp", "infer"),
                                         ("--mode eval --save_sp_guide", "save_sp_guide"),
                                         ("--mode eval --save_sp_guide --eval_no_sp", "save_sp_guide")])
def test_entry_refuses_predict_and_save_sp_guide_on_both_spatial_paths(tmp_path, extra, match):
    from boxsegliver_amd.entry import main as entry
    argv = ("liver --tag t --model GUNet --model_config GUNet_SP.yml --classes Liver Tumor --use_spatial "
            "--evaluator Volume --model_dir {} {}".format(tmp_path, extra)).split()
    args, sub, pipe = entry.get_arguments(argv, guided=True)
    with pytest.raises(NotImplementedError, match=match):
        entry.run(args, sub, pipe, guided=True)


@pytest.mark.parametrize("over,match", [(dict(real_sp="x.json"), "real_sp"), (dict(save_sp_guide=True), "save_sp_guide"),
                                        (dict(mode="infer"), "infer")])
def test_eval_no_sp_slabs_refuse_what_is_out_of_scope(over, match):
    from boxsegliver_amd.data import lits
    args = argparse.Namespace(real_sp=None, save_sp_guide=False, mode="eval", batch_size=2, im_height=8, im_width=8,
                              use_context=False)
    for k, v in over.items():
        setattr(args, k, v)
    with pytest.raises(NotImplementedError, match=match):
        lits.eval_no_sp_features(args)
