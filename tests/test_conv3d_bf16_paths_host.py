"""No GPU: the table of tests/test_gpu_conv3d_bf16_paths.py (tests/conv3d_bf16_cases.py) is self-consistent and its inputs can
tell a wrong kernel from a right one.

Every row's hand-written kernel names, statistic rows, tile geometry and filter-gradient splits agree with a Python restatement
of pick_bf16 / unetk_wgrad_plan / unetk_launch_slab_reduce; the table as a whole names every kernel the device test must reach; both
exact input sets are bf16-representable and stay inside the exact regime (so a table edit cannot leave it silently); and for
each way a fused-depth-tap kernel can plausibly be wrong -- depth taps leaking across samples, reversed, clamped instead of
zero-padded, one (tap, 32-channel chunk) step dropped, a missing plane's filter gradient copied from the middle tap -- the wrong
result differs from the float64 reference on the row's own inputs.

The true reference is oracle.tf_ops.conv_nd_same in float64.  The deliberately wrong ones are evaluated in float32, which is
exact on these inputs (test_float32_evaluation_is_exact_here shows it on the true convolution of every row); they only have to
differ.
"""
import pytest
import torch

import conv3d_bf16_cases as T
from oracle import tf_ops

CASES = T.CASES
IDS = [c.id for c in CASES]
EXACT_KINDS = ("eighths", "sparse")


def test_ids_are_unique():
    assert len(T.BY_ID) == len(CASES) == len(set(IDS))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_row_agrees_with_the_restated_predicates(case):
    c = case
    assert c.kd in (1, 3) and c.cin % 32 == 0 and c.cout % 32 == 0 and c.xpad % 4 == 0 and c.ypad % 4 == 0
    ft = c.kd == 3
    planes = c.n * c.d
    f = T.pick_bf16(c.h, c.cin, c.cout, planes, c.w)
    g = T.pick_bf16(c.h, c.cout, c.cin, planes, c.w)            # the input gradient contracts Cout into Cin
    assert c.fwd == T.bf(f, ft) and c.dgrad == T.bf(g, ft), (c.id, f, g)
    # the stated tile geometry is that configuration's and gives the stated statistic rows
    th, tiles_h, tiles_w = c.tiles
    assert th == T.CFG[f][1] and tiles_h == -(-c.h // th) and tiles_w == -(-c.w // T.TW)
    assert tiles_h * tiles_w * planes == c.rows and c.rows % c.n == 0
    cit, cot, s = T.wg_splits(planes, c.h, c.w, c.cin, c.cout, c.kd)
    want = [T.wg(cit, cot)] + ([T.reducer(s)] if s > 1 else [])
    assert s == c.splits and list(c.wgrad) == want, (c.id, s, want)


def test_table_names_every_required_kernel():
    """What the device test's closing test asks of the traces, asked of the table."""
    for cfg in range(5):
        assert any(c.fwd == T.bf(cfg, True) for c in CASES), cfg
        assert any(c.dgrad == T.bf(cfg, True) for c in CASES), cfg
        assert any(T.bf(cfg, False) in (c.fwd, c.dgrad) for c in CASES), cfg
    for cit in (64, 32):
        for cot in (64, 32):
            for kd in (3, 1):
                assert any(c.kd == kd and c.wgrad[0] == T.wg(cit, cot) for c in CASES), (cit, cot, kd)
    assert any(c.kd == 3 and len(c.wgrad) == 1 and c.splits == 1 for c in CASES)
    assert any(c.kd == 3 and len(c.wgrad) == 2 for c in CASES)
    # the depth edges: D = 1 alone and side by side, D = 2 with N > 1, a plane with partial tiles both ways, one below a tile
    assert any(c.kd == 3 and c.d == 1 and c.n == 1 for c in CASES) and any(c.kd == 3 and c.d == 1 and c.n > 1 for c in CASES)
    assert any(c.kd == 3 and c.d == 2 and c.n > 1 for c in CASES)
    assert any(c.kd == 3 and c.tiles[1] > 1 and c.tiles[2] > 1 and c.h % c.tiles[0] and c.w % T.TW for c in CASES)
    assert any(c.kd == 3 and c.h < c.tiles[0] and c.w < T.TW for c in CASES)
    # 512 x 128 exactly at its 200-block threshold
    assert any(c.fwd == T.bf(0, True) and c.rows * (c.cout // 128) == 200 for c in CASES)


@pytest.mark.parametrize("kind", T.KINDS[:2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_are_bf16_values_inside_the_exact_regime(case, kind):
    x, w, dy, lsb = T.make_inputs(case, kind)
    for t in (x, w, dy):
        assert torch.equal(t.bfloat16().float(), t)
    y64, _, _, amax = T.reference(case, kind)
    T.exact_bounds(case, kind, x, w, dy, lsb, y64, amax)
    if kind == "sparse":                                    # the statistic partials: whole-tile sums below 2^24
        th = case.tiles[0]
        assert th * T.TW * 15 * 15 < 2 ** 24
        s1, s2 = T.tile_stats(y64, case)
        assert tuple(s1.shape) == (case.rows, case.cout)
        assert torch.equal(s1.sum(0), y64.sum((0, 1, 2, 3))) and torch.equal(s2.sum(0), (y64 * y64).sum((0, 1, 2, 3)))


def _f32(case, kind, conv=tf_ops.conv_nd_same):
    x, w, dy, _ = T.make_inputs(case, kind)
    return [t.double() for t in T.conv_grads(x, w, dy, conv)]


@pytest.mark.parametrize("kind", EXACT_KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_evaluation_is_exact_here(case, kind):
    y64, dx64, dw64, _ = T.reference(case, kind)
    y, dx, dw = _f32(case, kind)
    assert torch.equal(y, y64) and torch.equal(dx, dx64) and torch.equal(dw, dw64)


def _leak(case):
    """depth taps leak across samples: the N D planes as one sample"""
    def conv(x, w):
        return tf_ops.conv_nd_same(x.reshape((1, case.n * case.d) + tuple(x.shape[2:])), w).reshape(
            tuple(x.shape[:4]) + (case.cout,))
    return conv


def _reversed(x, w):
    return tf_ops.conv_nd_same(x, w.flip(0))


def _clamped(x, w):
    """depth zero padding replaced by the edge plane"""
    xp = torch.cat((x[:, :1], x, x[:, -1:]), 1)
    return tf_ops.conv_nd_same(xp, w)[:, 1:-1]


def _dropped(case):
    """the last 32-channel chunk of the middle depth tap (the one every plane has) left out of the contraction"""
    def conv(x, w):
        keep = torch.ones_like(w)
        keep[case.kd // 2, :, :, case.cin - 32:, :] = 0
        return tf_ops.conv_nd_same(x, w * keep)
    return conv


@pytest.mark.parametrize("kind", EXACT_KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_discriminate(case, kind):
    y64, dx64, dw64, _ = T.reference(case, kind)
    true = {"y": y64, "dx": dx64, "dw": dw64}
    wrongs = [("dropped chunk", _dropped(case), ("y", "dx"))]
    if case.kd == 3 and case.n > 1:                           # kd = 1 has no depth taps to leak
        wrongs.append(("leak across samples", _leak(case), ("y", "dx", "dw")))
    if case.kd == 3 and case.d >= 2:
        wrongs.append(("reversed depth taps", _reversed, ("y", "dx", "dw")))
    if case.kd == 3:
        wrongs.append(("clamped depth edge", _clamped, ("y", "dx", "dw")))
    for what, conv, outs in wrongs:
        got = dict(zip(("y", "dx", "dw"), _f32(case, kind, conv)))
        for o in outs:
            assert got[o].shape == true[o].shape
            assert not torch.equal(got[o], true[o]), (case.id, kind, what, o)
    if case.kd == 3 and case.d == 1:
        # the taps without an input plane: exactly zero, and the middle tap is not (so a copy of it would show)
        assert float(dw64[0].abs().max()) == 0.0 and float(dw64[2].abs().max()) == 0.0
        assert float(dw64[1].abs().max()) > 0.0
