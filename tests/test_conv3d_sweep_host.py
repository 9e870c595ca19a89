"""No GPU: the sweep of tests/conv3d_sweep_cases.py is what test_gpu_conv3d_sweep.py needs it to be.

  * every branch of the composition has grid cases under the restatement of the dispatch, and the input gradient's dilated
    fallback (conv3d.hip, DGRAD_DILATED) has at least 100 in each stride-2 family;
  * every case is in the exact regime of its input kind, from its own float64 reference: fp32 sums are exact in any order, so the
    device test may ask for bit equality;
  * the host-callable queries of the library (pure host arithmetic) hold their contracts at every extent up to 40.
"""
import collections
import ctypes

import pytest
import torch

import conv3d_sweep_cases as S
from oracle import tf_ops

IDS = [S.item_id(i) for i in S.ITEMS]


def test_every_branch_has_grid_cases():
    count = collections.Counter()
    for item in S.ITEMS:
        for c in S.cases(*item):
            count.update(S.branch(c))
    assert set(count) == set(S.BRANCHES)
    assert all(count[b] >= 8 for b in S.BRANCHES), count


@pytest.mark.parametrize("family", S.STRIDE2_FAMILIES, ids=lambda f: "k{}s{}".format(f[0], "".join(map(str, f[1]))))
def test_dilated_dgrad_fallback_is_dense_on_the_full_grid(family):
    cs = [c for c in S.cases(family, S.CHANNELS[0]) if S.branch(c)[1] == S.D_DILATED]
    assert len(cs) >= 100
    assert {c.d % 2 for c in cs} == {0, 1}
    # the smallest shapes that reach it, and a dy plane of one row
    assert any((c.h, c.w) == (2, 2) for c in cs) and any((c.h, c.w) == (2, 33) for c in cs)


def test_grid_is_the_stated_one():
    assert len(S.extents(S.CHANNELS[0])) == 390 and len(S.extents(S.CHANNELS[1])) == 84 == len(S.extents(S.CHANNELS[2]))
    assert len(S.ITEMS) == 15
    for item in S.ITEMS:
        cs = S.cases(*item)
        assert all(c.n == 1 + (c.d + c.h + c.w) % 2 for c in cs)
        assert [c.sliced for c in cs] == [i % 2 == 1 for i in range(len(cs))]
        assert len({S.seed(c, k) for c in cs for k in ("eighths", "sparse")}) == 2 * len(cs)


@pytest.mark.parametrize("item", S.ITEMS, ids=IDS)
def test_exact_regime_of_every_case(item):
    worst_abs, worst_y, worst_sq = 0.0, 0.0, 0.0
    with torch.no_grad():
        for c in S.cases(*item):
            x, w, dy = S.make_inputs(c, "eighths")
            # y: every partial sum is a multiple of 1/8 below 2^24 / 8; dx likewise (|dy| <= 2, |w| <= 1/4 over 9 kd Cout
            # products); dw: integers x dy over the output pixels
            amax = tf_ops.conv_nd_same(x.abs(), w.abs(), stride=c.stride).max().item()
            worst_abs = max(worst_abs, amax)
            assert amax * 8 < 2 ** 24, S.case_id(c)
            assert 9 * c.kd * c.cout * 2 * 0.25 * 8 < 2 ** 24
            assert 8 * (dy.numel() // c.cout) < 2 ** 24, S.case_id(c)
            x, w, _ = S.make_inputs(c, "sparse")
            y = tf_ops.conv_nd_same(x, w, stride=c.stride)
            worst_y = max(worst_y, y.abs().max().item())
            assert y.abs().max().item() <= 15, S.case_id(c)
            sq = (y * y).sum((1, 2, 3)).max().item()      # the statistic partials: integer sums far below 2^24
            worst_sq = max(worst_sq, sq)
            assert sq < 2 ** 24, S.case_id(c)
    print("{}: max |x| conv |w| {}, sparse max |y| {}, max per-sample sum y^2 {}".format(S.item_id(item), worst_abs, worst_y, worst_sq))


@pytest.fixture(scope="module")
def L():
    from boxsegliver_amd import _abi
    return _abi.lib()


@pytest.mark.parametrize("channels", S.CHANNELS, ids=lambda c: "{}x{}".format(*c))
def test_host_queries_at_every_extent_up_to_40(L, channels):
    """unetk_conv3d_out_dims = ceil(extent / stride); unetk_conv3d_stat_rows > 0 and a multiple of N (each sample's rows are
    contiguous); unetk_conv3d_ws_bytes holds the stride-1 result / the dilated dy of a stride-2 layer (every stride-2 layer can
    take a scratch or dilated route: the filter gradient or the input gradient's fallback); nothing is refused."""
    from boxsegliver_amd import _abi
    cin, cout = channels
    do, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    pdo, pho, pwo = ctypes.byref(do), ctypes.byref(ho), ctypes.byref(wo)
    bad = []
    for kd, (sd, shw, _) in S.FAMILIES:
        d = _abi.Conv3dDesc(1, 1, 1, 1, cin, cout, kd, sd, shw, cin, cout)
        pd = ctypes.byref(d)
        for dd in range(1, 41):
            d.D = dd
            for h in range(1, 41):
                d.H = h
                for w in range(1, 41):
                    d.W = w
                    n = d.N = 2 + (dd + h + w) % 2
                    rc = L.unetk_conv3d_out_dims(pd, pdo, pho, pwo)
                    rows = L.unetk_conv3d_stat_rows(pd)
                    ws = L.unetk_conv3d_ws_bytes(pd)
                    ok = rc == 0 and (do.value, ho.value, wo.value) == (-(-dd // sd), -(-h // shw), -(-w // shw))
                    ok = ok and rows > 0 and rows % n == 0
                    ok = ok and (shw == 1 or ws >= n * do.value * h * w * cout * 4)
                    if not ok:
                        bad.append(((n, dd, h, w, cin, cout, kd, sd, shw), rc, (do.value, ho.value, wo.value), rows, ws))
    assert not bad, "{} descriptors, the first: {}".format(len(bad), bad[:5])
