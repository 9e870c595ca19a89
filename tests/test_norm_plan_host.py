"""No GPU: the two host queries of the normaliser family are the plan of the call (csrc/norm.hip norm_plan).

unetk_norm_bwd_ws_bytes is the segment-wise maximum of the one layout function every backward run lays its workspace out with,
and it is 0 exactly where norm_plan refuses the descriptor whatever optional operands come with it; unetk_norm_finalize_ws_bytes
uses the statistics geometry alone.  Both are pure host arithmetic.  They are held to

  * the Python restatement tests/norm_paths.py (ws_bytes) on every row of the GPU table, in both storages;
  * tests/golden/norm_plan_queries.npz, recorded by tests/golden/make_norm_plan_fixture.py from the library as it was BEFORE the
    plan existed (the query had its own formula and its own copy of the refusal rules): moving onto the plan changed no number;
  * the refusal table of tests/test_gpu_norm_paths.py: 0 where the descriptor alone decides, the valid shape's bytes elsewhere.

A descriptor is refused (or, by the finalise query, answered) before anything divides by a quantity it could make zero: the thread
map of C = 1..3 has C / 4 = 0 channel quads, that of C > 1024 has 256 / (C / 4) = 0 rows.  Those cases run in this process: a
trap ends the test run instead of passing.
"""
import importlib.util
import os

import numpy as np
import pytest

import norm_paths as T
from test_gpu_norm_paths import BASE, REFUSALS, make_desc

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_norm_plan_fixture", os.path.join(HERE, "golden", "make_norm_plan_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_generator()
STORAGES = (T.FP32S, T.BF16S)


@pytest.fixture(scope="module")
def L():
    return G.library()


@pytest.fixture(scope="module")
def recorded():
    z = np.load(G.OUT)
    for name, values in G.AXES:
        assert z["axis_" + name].tolist() == list(values), "the fixture was recorded for another sweep"
    assert z["row_factors"].tolist() == list(G.ROW_FACTORS)
    return z["bwd"], z["fin"]


# ------------------------------------------------------------------ the restated query
@pytest.mark.parametrize("row", T.ROWS, ids=[r.id for r in T.ROWS])
def test_backward_query_is_the_restated_formula(L, row):
    for st in STORAGES:
        assert G.ask_bwd(L, make_desc(row, st)) == T.ws_bytes(row) > 0, st


# ------------------------------------------------------------------ recorded values
def test_fixture_is_small_and_is_the_whole_sweep(recorded):
    bwd, fin = recorded
    assert os.path.getsize(G.OUT) < 100 * 1024
    assert bwd.shape == G.SHAPE == (5, 6, 9, 2, 5, 2) and fin.shape == G.SHAPE + (5,)


def test_queries_equal_the_values_recorded_before_the_plan(L, recorded):
    bwd, fin = recorded
    got_b, got_f = G.record(L)
    bad = np.argwhere(got_b != bwd)
    assert bad.size == 0, "backward query: {} of {} differ, first at {}".format(len(bad), bwd.size, bad[:3].tolist())
    bad = np.argwhere(got_f != fin)
    assert bad.size == 0, "finalise query: {} of {} differ, first at {}".format(len(bad), fin.size, bad[:3].tolist())


def test_recorded_values_are_not_trivial(recorded):
    bwd, fin = recorded
    assert (bwd > 0).all() and (fin > 0).all()
    # the reducer's first level (64 row blocks) starts above 256 rows per group: scratch appears between the factors 256 and 257
    assert (fin[..., 0] == fin[..., 2]).all() and (fin[..., 3] > fin[..., 2]).all() and (fin[..., 4] == fin[..., 3]).all()
    # storage never enters a size; the guide channels enter the backward's alone
    assert (bwd[..., 0] == bwd[..., 1]).all() and (fin[..., 0, :] == fin[..., 1, :]).all()
    assert (np.diff(bwd, axis=4) > 0).all() and (np.diff(fin, axis=4) == 0).all()
    # both cap regimes of bwd_blocks, each reached and not reached: 1024 blocks of one launch group, max(2048 / L, 64) of several
    seen = set()
    for n, hw, c, ps, _, _ in G.sweep():
        rpi = T.colmap(c)[1]
        for L_ in (n, n if ps else 1):                 # the density geometry and the plain one
            p = hw if L_ > 1 else n * hw
            rows = -(-p // rpi)
            seen.add(("one" if L_ == 1 else ("floor64" if 2048 // L_ <= 64 else "2048/L"), rows > T.bwd_blocks(p, rpi, L_)))
    assert seen == {(k, capped) for k in ("one", "floor64", "2048/L") for capped in (False, True)}, seen


# ------------------------------------------------------------------ refusals the descriptor alone decides
@pytest.mark.parametrize("name,rowo,desco,callo,codes,ws0", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_table_asks_for_nothing_or_for_the_valid_shape(L, name, rowo, desco, callo, codes, ws0):
    r = BASE._replace(id=name, **rowo)
    if r.g or r.gbare:
        r = r._replace(gstride=r.c)
    got = G.ask_bwd(L, make_desc(r, T.FP32S, guide_alpha=0.25, **desco))
    assert got == (0 if ws0 else T.ws_bytes(r)), (name, got)


# ------------------------------------------------------------------ refused or answered before anything divides
def _finalize_formula(n, hw, c, per_sample, stat_rows):
    """unetk_norm_finalize_ws_bytes restated: finalize_ws_base (sums + first-level row sums, rounded up to 16) and the
    refinement scratch part[Ns][cblocks][PB][2][16] + one[Ns][C][2] doubles, flags[Ns][C], counters[Ns][cblocks]."""
    ns = n if per_sample else 1
    ps = hw if per_sample else n * hw
    base = -(-4 * (2 * ns * c + T.tmp_floats(2 * ns, stat_rows // ns, c)) // 16) * 16
    cblocks = -(-c // 16)
    pb = min(max(-(-ps // 4096), 1), 64)
    return base + ns * cblocks * pb * 32 * 8 + ns * c * 2 * 8 + ns * c * 4 + ns * cblocks * 4


@pytest.mark.parametrize("c", [1, 2, 3])
def test_fewer_than_four_channels(L, c):
    """No thread map exists (C / 4 = 0 quads): the backward query refuses, the finalise kernels take any C > 0 and their query
    answers its formula -- 316 bytes at N = 1, HW = 16, C = 2, one stat row."""
    for n, hw, per_sample in ((1, 16, 0), (2, 16, 0), (2, 16, 1), (5, 884736, 1)):
        for st in STORAGES:
            d = G.desc(n, hw, c, per_sample, 0, st)
            assert G.ask_bwd(L, d) == 0
            ns = n if per_sample else 1
            for k in G.ROW_FACTORS:
                assert G.ask_finalize(L, d, k * ns) == _finalize_formula(n, hw, c, per_sample, k * ns) > 0
    assert G.ask_finalize(L, G.desc(1, 16, 2, 0, 0, T.FP32S), 1) == 316


@pytest.mark.parametrize("c", [1028, 2048, 4096])
def test_more_than_1024_channels(L, c):
    """256 / (C / 4) = 0 rows per block: the backward query refuses before the launch geometry exists; the finalise query answers."""
    for per_sample in (0, 1):
        d = G.desc(2, 16, c, per_sample, 0, T.FP32S)
        assert G.ask_bwd(L, d) == 0
        assert G.ask_finalize(L, d, 2) == _finalize_formula(2, 16, c, per_sample, 2) > 0


@pytest.mark.parametrize("edit", [dict(N=0), dict(HW=0), dict(C=0), dict(N=-1), dict(guide_ch=-1), dict(guide_ch=5)],
                         ids=lambda e: "-".join("%s%d" % kv for kv in e.items()))
def test_bad_descriptors_ask_for_nothing(L, edit):
    for per_sample in (0, 1):
        for st in STORAGES:
            d = G.desc(2, 16, 24, per_sample, 0, st, **edit)
            assert G.ask_bwd(L, d) == 0 and G.ask_finalize(L, d, 2) == 0
    assert G.ask_finalize(L, G.desc(2, 16, 24, 0, 0, T.FP32S), 0) == 0 and G.ask_finalize(L, G.desc(2, 16, 24, 0, 0, T.FP32S), -2) == 0
