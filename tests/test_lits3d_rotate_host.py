"""CPU: `liver_3d --random_rotate` -- the two flags, the sampler's rotation draw and what it writes into the
table, the generator left alone when the feature is off (held to tables recorded before the flag existed,
tests/golden/lits3d_rotate_off.npz), the quarter-turn identities of the restatement, and the accumulate wrappers' refusal of a
rotated row."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import lits3d_ref as ref
import lits3d_rotate_ref as rref

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = ("liver_3d --mode train --tag t --model UNet3D --classes Liver Tumor --im_depth 6 --im_height 16 --im_width 20 "
        "--lits_root /data/LiTS").split()


def _fixtures():
    spec = importlib.util.spec_from_file_location("make_lits3d_rotate_fixtures",
                                                  os.path.join(HERE, "golden", "make_lits3d_rotate_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(extra=""):
    from boxsegliver_amd.entry import main as entry
    return entry.get_arguments(BASE + extra.split())[0]


# ------------------------------------------------------------------------------------------------- flags
def test_flag_defaults_and_parsing():
    from boxsegliver_amd.data import lits3d
    d = _args()
    assert d.random_rotate == 0.0 and d.rotate_prob == 1.0 and lits3d.rotation(d) == (0.0, 1.0)
    a = _args("--random_rotate 20 --rotate_prob 0.25")
    assert lits3d.rotation(a) == (20.0, 0.25) and lits3d.check_args(a) == (2, 2)
    assert lits3d.rotation(_args("--random_rotate 180 --rotate_prob 0")) == (180.0, 0.0)
    # the interactive evaluator shares the argument group: it parses the flags (and never rotates)
    from boxsegliver_amd.entry import main_eval_3d
    e = main_eval_3d.build_parser().parse_args(BASE[1:] + "--random_rotate 20 --rotate_prob 0.5".split())
    assert (e.random_rotate, e.rotate_prob) == (20.0, 0.5)
    e.random_rotate = 200.0
    with pytest.raises(ValueError, match="--random_rotate"):
        lits3d.check_values(e)


@pytest.mark.parametrize("extra,match", [("--random_rotate -1", "--random_rotate"), ("--random_rotate 180.5", "--random_rotate"),
                                         ("--random_rotate nan", "--random_rotate"), ("--rotate_prob -0.1", "--rotate_prob"),
                                         ("--rotate_prob 1.5", "--rotate_prob"), ("--rotate_prob nan", "--rotate_prob"),
                                         ("--random_rotate inf", "--random_rotate")])
def test_check_values_refuses_and_names_the_flag(extra, match):
    from boxsegliver_amd.data import lits3d
    with pytest.raises(ValueError, match=match):
        lits3d.check_values(_args(extra))


# ------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("config", ["unguided", "guided"])
def test_feature_off_uploads_the_recorded_tables(config):
    """The first three batches without the flag (and with --random_rotate 0) are, bit for bit, what the pipeline uploaded
    before the flag existed; columns 13..15 are zero and no wrapper is asked to rotate."""
    fx = _fixtures()
    gold = np.load(os.path.join(HERE, "golden", "lits3d_rotate_off.npz"))
    for kw in ({}, dict(random_rotate=0.0), dict(random_rotate=0.0, rotate_prob=0.3)):
        tabs, ctabs, calls = fx.stream(fx.CONFIGS[config], **kw)
        np.testing.assert_array_equal(tabs, gold[config + "_tab"])
        assert tabs.dtype == np.int32 and not tabs[:, :, 13:].any()
        if config == "guided":
            np.testing.assert_array_equal(ctabs, gold["guided_clicks"])
        else:
            assert ctabs is None
        assert all(not k.get("rotate", False) for _, k in calls)


@pytest.mark.parametrize("config", ["unguided", "guided"])
def test_rotation_draw_comes_last_and_fills_columns_13_14(config):
    fx = _fixtures()
    gold = np.load(os.path.join(HERE, "golden", "lits3d_rotate_off.npz"))
    tabs, ctabs, calls = fx.stream(fx.CONFIGS[config], random_rotate=30.0)
    np.testing.assert_array_equal(tabs[0][:, :13], gold[config + "_tab"][0][:, :13])    # the first batch's other draws stand
    if config == "guided":
        np.testing.assert_array_equal(ctabs[0], gold["guided_clicks"][0])               # the click draws come before it too
    assert not np.array_equal(tabs[1:, :, :13], gold[config + "_tab"][1:, :, :13])     # later batches: the generator moved on
    assert not tabs[:, :, 15].any()
    sc = np.ascontiguousarray(tabs[:, :, 13:15]).view(np.float32).astype(np.float64)
    assert np.all((tabs[:, :, 13] != 0) | (tabs[:, :, 14] != 0))                        # P = 1: every row rotated
    assert np.abs(sc[..., 0] ** 2 + sc[..., 1] ** 2 - 1.0).max() <= 4 * 2.0 ** -24      # two float32 roundings of values <= 1
    deg = np.rad2deg(np.arctan2(sc[..., 0], sc[..., 1]))
    assert np.all(np.abs(deg) <= 30.0 + 1e-4) and len(np.unique(deg)) == deg.size
    rotating = [k for name, k in calls if name in ("lits_patch3d", "click_guide3d")]
    assert len(rotating) == (6 if config == "guided" else 3) and all(k.get("rotate") is True for k in rotating)


def test_probability_zero_and_evaluation_leave_zeros():
    fx = _fixtures()
    tabs, _, calls = fx.stream(None, random_rotate=45.0, rotate_prob=0.0)
    assert not tabs[:, :, 13:].any()
    assert all(k.get("rotate") is True for name, k in calls if name == "lits_patch3d")  # the sampler rotates; no row drew it
    tabs, _, calls = fx.stream(None, random_rotate=45.0, training=False)                # eval_online: never
    assert not tabs[:, :, 13:].any() and all(not k.get("rotate", False) for _, k in calls)
    s = fx.sampler(random_rotate=45.0, training=False)
    assert s.rotate == 0.0 and s.draw_rotation() is None
    # a share of the rows at 0 < P < 1, zeros elsewhere
    s = fx.sampler(bs=2, random_rotate=45.0, rotate_prob=0.5, seed=3)
    on = np.concatenate([(s.table()[:, 13:15] != 0).any(axis=1) for _ in range(200)])
    assert 0.35 < on.mean() < 0.65


def test_table_takes_sin_and_cos_from_float64():
    fx = _fixtures()
    s = fx.sampler(bs=2, random_rotate=10.0)
    b = s.draw()
    tab = s.table(b, dict(on=np.array([True, False]), deg=np.array([90.0, 33.0])))
    assert tuple(tab[0, 13:15]) == (rref.bits(1.0), rref.bits(np.float32(np.cos(np.pi / 2))))
    assert tuple(tab[1, 13:16]) == (0, 0, 0)
    np.testing.assert_array_equal(tab[:, :13], s.table(b)[:, :13])
    assert rref.sincos(90.0) == (np.float32(1.0), np.float32(np.cos(np.pi / 2)))


def test_eval_tables_never_rotate():
    from boxsegliver_amd.data import lits3d

    class Store(object):
        im = torch.zeros((sum(ref.DEPTHS), ref.H, ref.W), dtype=torch.int16)
        offset = {0: 0}
    for tab in lits3d.eval_tables({"PID": 0, "size": [ref.DEPTHS[0], ref.H, ref.W]}, Store(), (6, 16, 20), 0.5, [(0, 0, 0), (1, 0, 0)], 4):
        assert not tab[:, 13:].any()


# ------------------------------------------------------------------------------------------------- the restatement
def test_restatement_quarter_turns_are_exact():
    """Square crop at zoom 1: (sin, cos) = (1, 0), (0, -1), (-1, 0) are np.rot90 by 3, 2, 1 and (0, 1) is the crop, bit for bit
    (image and label), against lits3d_ref.patch."""
    cases = ref.make_cases()
    shape = (6, 16, 16)
    for ci, centre in ((0, (6, 19, 23)), (0, (0, 0, 0)), (2, (2, 17, 21)), (3, (5, 39, 47))):
        im, lab = cases[ci]
        want, want_lab, m, s = ref.patch(im, lab, centre, (16, 16), shape)
        for sc, k in (((0.0, 1.0), 0), ((1.0, 0.0), 3), ((0.0, -1.0), 2), ((-1.0, 0.0), 1)):
            got, got_lab, gm, gs = rref.patch(im, lab, centre, (16, 16), shape, sc)
            assert (gm, gs) == (m, s)
            np.testing.assert_array_equal(got, np.rot90(want, k, axes=(1, 2)), err_msg=str((ci, centre, sc)))
            np.testing.assert_array_equal(got_lab, np.rot90(want_lab, k, axes=(1, 2)))
    # flips are applied after the turn
    got = rref.patch(im, lab, centre, (16, 16), shape, (1.0, 0.0), flips=(1, 0, 1))[0]
    np.testing.assert_array_equal(got, ref.flip(np.rot90(want, 3, axes=(1, 2)), (1, 0, 1)))


def test_restatement_coordinates_and_invalid_rows():
    in_y, in_x, ok = rref.coords((16, 20), (19, 23), rref.sincos(45.0))
    assert in_y.dtype == in_x.dtype == np.float32 and ok.all()
    # the centre of the patch maps to the centre of the crop for any angle
    cy, cx, _ = rref.coords((17, 21), (19, 23), rref.sincos(-33.0))
    assert cy[8, 10] == 9.0 and cx[8, 10] == 11.0
    for sc in ((np.nan, 1.0), (np.inf, 0.0), (0.0, -np.inf), (1e30, 1e30)):
        _, _, ok = rref.coords((16, 20), (19, 23), sc)
        assert not ok.all()
    cases = ref.make_cases()
    info = {}
    out, lb, _, _ = rref.patch(cases[0][0], cases[0][1], (6, 19, 23), (19, 23), (6, 16, 20), (1e30, 0.0), info=info)
    assert np.all(np.isfinite(out)) and info["invalid"] > 0 and not lb[:, np.broadcast_to(~rref.coords((16, 20), (19, 23), (1e30, 0.0))[2], (16, 20))].any()
    # roundf: half away from zero on both signs
    np.testing.assert_array_equal(rref._roundf(np.array([-1.5, -0.5, -0.49, 0.5, 1.5, 2.49], np.float32)), [-2, -1, 0, 1, 2, 2])


# ------------------------------------------------------------------------------------------------- the wrappers
def test_the_library_exports_the_rot_entry_points_and_checks_their_arguments():
    """Every refusal returns before anything is launched."""
    import ctypes
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    for name in ("unetk_lits_patch3d_rot", "unetk_click_guide3d_rot"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.unetk_abi_version() == 10                                             # additive
    d = _abi.Lits3dDesc(4, 10, 256, 256, 1000, 512, 512, 64, 64, 2, 1)
    nbytes = lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(d))
    assert nbytes > 0
    p = ctypes.c_void_p(1 << 20)                                                     # never dereferenced: the calls return first
    assert lib.unetk_lits_patch3d_rot(ctypes.byref(d), p, p, p, p, p, p, nbytes - 1, None) == -3      # UNETK_E_WORKSPACE
    assert lib.unetk_lits_patch3d_rot(ctypes.byref(d), p, p, None, p, p, p, nbytes, None) == -1       # UNETK_E_BADARG
    assert lib.unetk_lits_patch3d_rot(ctypes.byref(d), p, p, p, p, p, ctypes.c_void_p((1 << 20) + 8), nbytes, None) == -1
    big = _abi.Lits3dDesc(1, 2048, 1024, 1024, 1000, 512, 512, 64, 64, 2, 0)
    assert lib.unetk_lits_patch3d_rot(ctypes.byref(big), p, p, p, p, p, p, 1 << 30, None) == -2        # UNETK_E_UNSUPPORTED
    g = _abi.Lits3dClicksDesc(N=4, D=10, H=256, W=256, n_slices=1000, src_h=512, src_w=512, lab_scale=64, obj_label=2, margin=3,
                              step=10, band=40, max_clicks=5, G=2, gaussian=1, stddev=(ctypes.c_float * 3)(1, 3, 3), euclid_norm=1.0)
    assert lib.unetk_click_guide3d_rot(ctypes.byref(g), p, p, p, None, None) == -1
    assert lib.unetk_click_guide3d_rot(ctypes.byref(g), p, p, p, ctypes.c_void_p((1 << 20) + 2), None) == -1
    g.G = 3
    assert lib.unetk_click_guide3d_rot(ctypes.byref(g), p, p, p, p, None) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_refuses_a_rotated_row(weighted):
    """The wrapper needs device tensors, so this part runs on the GPU: nothing is launched for the refused table."""
    from boxsegliver_amd import ops
    shape, c = (6, 16, 20), 2
    cases = ref.make_cases()
    im, _, base = ref.stack_store(cases)
    slices = torch.from_numpy(im.view(np.int16)).cuda()
    depth = ref.DEPTHS[0]
    rows = np.stack([rref.table_row(base[0], depth, (3, 20, 24), (18, 22)),
                     rref.table_row(base[0], depth, (3, 20, 24), (18, 22), sc=(0.0, 1.0))])
    probs = torch.zeros((2,) + shape + (c,), device="cuda")
    acc = torch.zeros((depth, ref.H, ref.W, c), device="cuda")
    weight = torch.zeros((depth, ref.H, ref.W), dtype=torch.float32 if weighted else torch.int32, device="cuda")
    box = (0, 6, 11, 29, 13, 35)
    tables = tuple(torch.ones(n, device="cuda") for n in shape)

    def call(host):
        tab = torch.from_numpy(host).cuda()
        if weighted:
            return ops.eval3d_accumulate_w(probs, tab, shape, int(base[0]), depth, box, tables, acc, weight, slices, host_tab=host)
        return ops.eval3d_accumulate(probs, tab, shape, int(base[0]), depth, box, acc, weight, slices, host_tab=host)
    with pytest.raises(ValueError, match="rotat"):
        call(rows)
    only_sin = rows.copy()
    only_sin[1, 14] = 0
    only_sin[1, 13] = rref.bits(-0.0)
    with pytest.raises(ValueError, match="rotat"):
        call(only_sin)
    torch.cuda.synchronize()
    assert not bool(acc.any()) and not bool(weight.any())
    call(np.stack([rows[0], rows[0]]))                                               # the same rows without the columns pass
    torch.cuda.synchronize()
    assert bool((weight > 0).any())
