"""CPU: the definition of the geodesic click guide (tests/lits_geodesic_ref.py) and the `--geodesic_guide` flag.

The distance is builder-defined, so the first thing to show is that it IS a definition: a heap Dijkstra and a Jacobi
relaxation, two orders that share nothing but the float32 operations, end at the same bits on every field the GPU tests use."""
import argparse

import numpy as np
import pytest

import lits_geodesic_ref as ref

F = np.float32


def _fields():
    """(name, field, seeds): the grids, fields and seed sets of tests/test_gpu_lits_geodesic.py."""
    out = []
    for h, w in ((1, 1), (1, 5), (5, 1), (5, 4), (8, 8), (37, 23)):
        rng = np.random.default_rng(100 * h + w)
        corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
        many = [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(20)]
        for name, f in (("normal", ref.field_normal(h, w, seed=h * w)), ("constant", ref.field_constant(h, w)),
                        ("step", ref.field_step(h, w))):
            out.append(("{} {}x{} one".format(name, h, w), f, [(h // 2, w // 3)]))
            out.append(("{} {}x{} corners".format(name, h, w), f, corners))
            out.append(("{} {}x{} 64 with duplicates".format(name, h, w), f, (many + many + many + corners)[:64]))
    out.append(("maze corner", ref.field_maze(33), [(0, 0)]))
    out.append(("maze two", ref.field_maze(33), [(0, 0), (32, 0)]))
    return out


FIELDS = _fields()


@pytest.mark.parametrize("name,field,seeds", FIELDS, ids=[f[0] for f in FIELDS])
def test_dijkstra_and_jacobi_agree_bit_for_bit(name, field, seeds):
    """The uniqueness claim of the definition, demonstrated: every relaxation order ends at the same float32 bits."""
    d = ref.dijkstra(field, seeds)
    j, sweeps = ref.jacobi(field, seeds)
    assert d.dtype == np.float32 and j.dtype == np.float32 and np.all(np.isfinite(d))
    np.testing.assert_array_equal(d.view(np.int32), j.view(np.int32))
    assert sweeps < field.size                                          # Bellman-Ford: fewer productive sweeps than pixels
    for y, x in seeds:
        assert d[y, x] == 0
    assert (d == 0).sum() == len(set(seeds))                            # c >= 1: nothing else is at distance 0


def test_no_seed_is_exactly_zero():
    assert not ref.dijkstra(ref.field_normal(5, 4), []).any() and not ref.jacobi(ref.field_normal(5, 4), [])[0].any()


def test_the_maze_needs_more_sweeps_than_any_fixed_small_count():
    """On the 33 x 33 spiral the cheap way from the corner winds through the corridor: a solver with a sweep count tied to the
    grid's extent stops far short, so the GPU twin of this field cannot pass on one."""
    maze = ref.field_maze(33)
    assert maze.shape == (33, 33) and set(np.unique(maze).tolist()) == {0.0, 1000.0}
    full, sweeps = ref.jacobi(maze, [(0, 0)])
    assert sweeps > 4 * 33
    short, _ = ref.jacobi(maze, [(0, 0)], max_sweeps=4 * 33)
    assert not np.array_equal(full, short)
    # the corridor is followed: its far end is nearer through the corridor than across one wall
    corridor = full[maze == 0]
    assert corridor.max() < 1000 and corridor.max() > 4 * 33


def test_constant_field_gives_the_float32_chamfer_sums():
    """dI = 0: every step costs 1 or sqrtf(2), and a shortest path takes nd = min(|dy|, |dx|) diagonal steps and na = the rest
    axial ones (any other multiset is longer by 2 - sqrt(2) at least, far above the rounding of these sums).  The float32 sum
    depends on the order of the steps and the definition takes the least: chamfer[i][j] = min(fl(chamfer[i - 1][j] + sqrtf(2)),
    fl(chamfer[i][j - 1] + 1)), float addition being monotone.  D equals it exactly."""
    h, w = 37, 23
    seed = (5, 7)
    d = ref.dijkstra(ref.field_constant(h, w, 2.5), [seed])
    r2 = np.sqrt(F(2.0))
    n = max(h, w)
    chamfer = np.full((n, n), np.inf, F)
    chamfer[0, 0] = 0
    for i in range(n):
        for j in range(n):
            if i > 0:
                chamfer[i, j] = min(chamfer[i, j], F(chamfer[i - 1, j] + r2))
            if j > 0:
                chamfer[i, j] = min(chamfer[i, j], F(chamfer[i, j - 1] + F(1)))
    for y in range(h):
        for x in range(w):
            a, b = abs(y - seed[0]), abs(x - seed[1])
            assert d[y, x] == chamfer[min(a, b), max(a, b) - min(a, b)], (y, x)
    for k in range(1, 15):                                              # pure runs: one order
        assert d[seed[0], seed[1] + k] == F(k) and d[seed[0] + k, seed[1]] == F(k)
    acc = F(0)
    for k in range(1, 15):
        acc = F(acc + r2)
        assert d[seed[0] + k, seed[1] + k] == acc


@pytest.mark.parametrize("h", [24, 25, 64, 65])
@pytest.mark.parametrize("ch", [17, 40, 100])
def test_seed_mapping(h, ch):
    """:483 in float32: H odd and even, crops below and above H, the last row of the crop, clamping."""
    hh = (h + 1) // 2
    for y in (0, 1, ch // 2, ch - 2, ch - 1):
        want = int(F(F(F(y) / F(ch)) * F(h)) / F(2))
        assert ref.seed_index(y, ch, h, hh) == min(want, hh - 1)
        assert abs(ref.seed_index(y, ch, h, hh) - y * h / ch / 2) <= 1
    assert ref.seed_index(ch - 1, ch, h, hh) <= hh - 1
    assert ref.seed_index(ch - 1, ch, h, hh) == min(int(np.floor((ch - 1) * h / ch / 2 + 1e-4)), hh - 1)
    assert ref.seed_index(-3, ch, h, hh) == 0 and ref.seed_index(10 * ch, ch, h, hh) == hh - 1      # clamped into the grid
    assert ref.seeds_of(np.array([[0, 0], [ch - 1, ch - 1], [5, 5]]), 2, (ch, ch), (h, h)) == \
        [(0, 0), (ref.seed_index(ch - 1, ch, h, hh),) * 2]
    assert ref.seeds_of(np.array([[0, 0]]), 7, (ch, ch), (h, h)) == [(0, 0)]                       # cnt clamped into [0, K]
    assert ref.seeds_of(np.array([[0, 0]]), -1, (ch, ch), (h, h)) == []


def test_odd_output_resize_keeps_the_distances_at_even_pixels():
    d = ref.dijkstra(ref.field_normal(5, 4, seed=3), [(1, 1)])
    g = ref.resize(d, (9, 7))
    np.testing.assert_array_equal(g[::2, ::2], d.astype(np.float64))


# ------------------------------------------------------------------------------------------------- flags
def _train_argv(extra):
    return ("liver_inter --mode train --tag t --model UNetInter --classes Tumor --im_height 32 --im_width 32 --im_channel 3 "
            "--batch_size 2 --lits_root data/LiTS").split() + list(extra)


def _eval_argv(extra):
    return ("--mode eval --tag t --model UNetInter --classes Tumor --im_height 32 --im_width 32 --lits_root data/LiTS").split() + list(extra)


def test_geodesic_guide_parses_for_liver_inter_and_main_eval():
    from boxsegliver_amd.data import lits_inter
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval
    for guided in (False, True):
        args, sub, _ = entry.get_arguments(_train_argv(["--use_spatial", "--geodesic_guide"]), guided=guided)
        assert sub == "liver_inter" and args.geodesic_guide and args.use_spatial and not args.geodesic
        assert lits_inter.check_args(args) == 2
        assert not entry.get_arguments(_train_argv(["--use_spatial"]), guided=guided)[0].geodesic_guide
    # --local_enhance and --stddev are accepted and ignored under it
    args, _, _ = entry.get_arguments(_train_argv(["--use_spatial", "--geodesic_guide", "--local_enhance", "--stddev", "5"]), guided=True)
    assert lits_inter.check_args(args) == 2
    args = main_eval.get_arguments(_eval_argv(["--use_spatial", "--geodesic_guide"]))
    assert args.geodesic_guide and main_eval.check_args(args) == 2
    assert not main_eval.get_arguments(_eval_argv(["--use_spatial"])).geodesic_guide


def test_geodesic_is_still_refused_by_name():
    from boxsegliver_amd.data import lits_inter
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval
    args, _, _ = entry.get_arguments(_train_argv(["--use_spatial", "--geodesic"]), guided=True)
    with pytest.raises(NotImplementedError, match="--geodesic is not built"):
        lits_inter.check_args(args)
    args, _, _ = entry.get_arguments(_train_argv(["--use_spatial", "--geodesic", "--geodesic_guide"]), guided=True)
    with pytest.raises(NotImplementedError, match="--geodesic is not built"):
        lits_inter.check_args(args)
    with pytest.raises(NotImplementedError, match="--geodesic is not built"):
        main_eval.check_args(main_eval.get_arguments(_eval_argv(["--use_spatial", "--geodesic"])))


def test_geodesic_guide_needs_use_spatial():
    from boxsegliver_amd.data import lits_inter
    from boxsegliver_amd.entry import main as entry
    from boxsegliver_amd.entry import main_eval
    args, _, _ = entry.get_arguments(_train_argv(["--geodesic_guide"]), guided=True)
    with pytest.raises(ValueError, match="--geodesic_guide needs --use_spatial"):
        lits_inter.check_args(args)
    with pytest.raises(ValueError, match="--geodesic_guide needs --use_spatial"):
        main_eval.check_args(main_eval.get_arguments(_eval_argv(["--geodesic_guide"])))
    with pytest.raises(ValueError, match="--geodesic_guide.*--use_spatial"):
        lits_inter.check_values(argparse.Namespace(classes=["Tumor"], im_channel=3, geodesic_guide=True))


def test_the_flag_group_is_still_nf_inters():
    from boxsegliver_amd.data import flagsets, lits_inter
    assert flagsets.PIPELINES["liver_inter"] == flagsets.PIPELINES["nf_g_simply"]
    assert "--geodesic_guide" not in flagsets.PIPELINES["liver_inter"][0]
    assert (8, "a geodesic guide reached its sweep bound before it converged") in lits_inter.STATUS_BITS
