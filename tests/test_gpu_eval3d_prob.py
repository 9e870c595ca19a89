"""GPU: `unetk_eval3d_prob` (csrc/evalio.hip) -- one class of a sliding-window case's accumulator as a uint8
probability volume in NIfTI file order, against the float64 restatement infer3d_ref.prob.  acc, the weight and dst lie between
guardbuf guard bands.

Tolerance of the random-input test: the kernel rounds twice in fp32 (the division, the product with 255), which moves 255 p by
at most 255 * 2 * 2^-24 ~ 3.1e-5 relative to the float64 value; q must equal the restatement wherever 255 p lies farther than
2^-14 (twice that) from a half-integer, and differ by at most 1 elsewhere.  The share of such voxels is computed from the
restatement before the kernel runs and must stay below 1 % (it is about 1e-4 for uniform inputs)."""
import ctypes

import numpy as np
import pytest
import torch

import guardbuf
import infer3d_ref as iref

pytestmark = pytest.mark.gpu

VOL = (5, 13, 19)                           # (d, h, w): file shape (19, 13, 5) with the LiTS orientation
C = 3
FILL = 77


def _setup(acc, weight):
    """acc f32 [d,h,w,C] and weight (f32 or int32 [d,h,w]) as guarded inputs, dst uint8 as a guarded output."""
    g = dict(acc=guardbuf.guarded_input(torch.from_numpy(acc).cuda()))
    w = torch.from_numpy(weight).cuda()
    g["w"] = guardbuf.guarded_input(w.view(torch.float32).unsqueeze(-1))                     # int32 weights: their bit patterns
    n = int(np.prod(weight.shape))
    g["dst"] = guardbuf.GuardedWorkspace(n)
    g["dst"].fill(FILL)
    return g, n


def _run(g, n, weight, cls, box, tb, bits, c=C, shape=None):
    from boxsegliver_amd import _abi
    P = ctypes.c_void_p
    d, h, w = shape or weight.shape
    is_w = weight.dtype == np.float32
    cbox = (ctypes.c_int32 * 6)(*box) if box is not None else None
    rc = _abi.lib().unetk_eval3d_prob(P(g["acc"].ptr()), c, cls, d, h, w, P(g["w"].ptr()) if is_w else None,
                                      None if is_w else P(g["w"].ptr()), cbox, tb[0], tb[1], tb[2], bits, P(g["dst"].ptr()),
                                      _abi.stream_ptr())
    torch.cuda.synchronize()
    ws = g["dst"]
    return rc, ws.buf[ws.off:ws.off + n].cpu().numpy()


def _flips(bits):
    return (bool(bits & 1), bool(bits & 2), bool(bits & 4))


def _intact(g):
    return g["acc"].changed_anywhere() == 0 and g["w"].changed_anywhere() == 0 and g["dst"].guard_intact()


def _exact_inputs(kind, seed=0):
    """acc = small multiples of 2^-k, weights powers of two: p, 255 p and the rounding are exact in fp32 and in float64."""
    rng = np.random.default_rng(seed)
    wexp = rng.integers(0, 4, VOL)
    weight = (2.0 ** wexp).astype(np.float32) if kind == "wsum" else (1 << wexp).astype(np.int32)
    # p = m / 512 with m in 0..512: both ends, and the exact tie 255 * 256 / 512 = 127.5 (-> 128, to even), in every class
    m = rng.integers(0, 513, VOL + (C,))
    for x, v in enumerate((0, 512, 256, 1, 511, 255, 257, 384)):
        m[0, 0, x, :] = v
    acc = (m / 512.0 * weight.astype(np.float64)[..., None]).astype(np.float32)
    return acc, weight


@pytest.mark.parametrize("kind", ["wsum", "cnt"])
def test_exact_inputs_match_everywhere(kind):
    acc, weight = _exact_inputs(kind)
    g, n = _setup(acc, weight)
    whole = (0, VOL[0], 0, VOL[1], 0, VOL[2])
    for cls in range(C):
        t, want = iref.prob(acc, weight, cls)
        assert (np.abs(t - np.rint(t)) == 0.5).sum() > 0 and want.min() == 0 and want.max() == 255      # ties, both ends
        rc, got = _run(g, n, weight, cls, whole, (2, 1, 0), 0)
        assert rc == 0
        np.testing.assert_array_equal(got, iref.file_order(want, (2, 1, 0), _flips(0)))
        assert _intact(g)
    rc, again = _run(g, n, weight, C - 1, whole, (2, 1, 0), 0)
    assert rc == 0 and again.tobytes() == got.tobytes()                                     # two calls, identical bits


@pytest.mark.parametrize("kind", ["wsum", "cnt"])
def test_holes_and_a_box_give_zero(kind):
    acc, weight = _exact_inputs(kind, seed=3)
    acc += np.float32(0.25) * weight[..., None].astype(np.float32)                          # no zero probabilities by chance
    holes = np.random.default_rng(8).random(VOL) < 0.2
    weight[holes] = 0
    weight[1, 2, 3] = -1 if kind == "cnt" else -0.5                                         # not > 0: uncovered
    box = (1, 4, 2, 11, 3, 17)
    g, n = _setup(acc, weight)
    t, want = iref.prob(acc, weight, 1, box)
    inside = np.zeros(VOL, bool)
    inside[1:4, 2:11, 3:17] = True
    assert (want[~inside] == 0).all() and (want[holes] == 0).all() and want[1, 2, 3] == 0 and (want[inside & ~holes] > 0).sum() > 100
    for tb, bits in (((2, 1, 0), 0), ((2, 1, 0), 7), ((0, 2, 1), 2)):
        rc, got = _run(g, n, weight, 1, box, tb, bits)
        assert rc == 0
        np.testing.assert_array_equal(got, iref.file_order(want, tb, _flips(bits)))
    assert _intact(g)


@pytest.mark.parametrize("tb", iref.PERMS)
def test_every_orientation(tb):
    acc, weight = _exact_inputs("wsum", seed=5)
    g, n = _setup(acc, weight)
    box = (0, 5, 1, 13, 0, 18)
    _, want = iref.prob(acc, weight, 2, box)
    seen = set()
    for bits in range(8):
        rc, got = _run(g, n, weight, 2, box, tb, bits)
        assert rc == 0
        np.testing.assert_array_equal(got, iref.file_order(want, tb, _flips(bits)), err_msg="{} {}".format(tb, bits))
        seen.add(got.tobytes())
    assert len(seen) == 8 and _intact(g)


def test_random_inputs_within_the_rounding_bound():
    rng = np.random.default_rng(17)
    vol = (6, 40, 48)
    wsum = rng.uniform(0.5, 8.0, vol).astype(np.float32)
    acc = (rng.random(vol + (C,)) * wsum[..., None]).astype(np.float32)
    acc = np.minimum(acc, wsum[..., None])
    # the restatement first: which voxels are too close to a tie to demand equality, and how many there are
    refs = [iref.prob(acc, wsum, cls) for cls in range(C)]
    near = [np.abs((t - np.floor(t)) - 0.5) <= 2.0 ** -14 for t, _ in refs]
    share = sum(int(m.sum()) for m in near) / float(C * wsum.size)
    print("voxels within 2^-14 of a half-integer: {:.3g} of {}".format(share, C * wsum.size))
    assert share <= 0.01
    g, n = _setup(acc, wsum)
    for cls, ((t, want), close) in enumerate(zip(refs, near)):
        rc, got = _run(g, n, wsum, cls, (0, vol[0], 0, vol[1], 0, vol[2]), (2, 1, 0), 1)
        assert rc == 0
        got = got.astype(np.int64)
        ref = iref.file_order(want, (2, 1, 0), _flips(1)).astype(np.int64)
        loose = iref.file_order(close, (2, 1, 0), _flips(1))
        print("class {}: max |q - ref| = {}, differing voxels = {}".format(cls, int(np.abs(got - ref).max()), int((got != ref).sum())))
        np.testing.assert_array_equal(got[~loose], ref[~loose])
        assert np.abs(got - ref).max() <= 1
    assert _intact(g)


def test_refused_calls_write_nothing():
    acc, weight = _exact_inputs("wsum")
    g, n = _setup(acc, weight)
    cnt = guardbuf.guarded_input(torch.ones(VOL + (1,), dtype=torch.int32, device="cuda").view(torch.float32))
    from boxsegliver_amd import _abi
    P = ctypes.c_void_p
    whole = (0, VOL[0], 0, VOL[1], 0, VOL[2])
    ok = dict(a=g["acc"].ptr(), C=C, c=1, d=VOL[0], h=VOL[1], w=VOL[2], ws=g["w"].ptr(), k=None, b=whole, tb=(2, 1, 0), f=0,
              o=g["dst"].ptr())

    def rc(**kw):
        v = dict(ok, **kw)
        box = (ctypes.c_int32 * 6)(*v["b"]) if v["b"] is not None else None
        r = _abi.lib().unetk_eval3d_prob(P(v["a"]), v["C"], v["c"], v["d"], v["h"], v["w"], P(v["ws"]), P(v["k"]), box,
                                         v["tb"][0], v["tb"][1], v["tb"][2], v["f"], P(v["o"]), _abi.stream_ptr())
        torch.cuda.synchronize()
        return r
    bad = [dict(a=None), dict(o=None), dict(b=None), dict(ws=None), dict(k=cnt.ptr()), dict(C=0), dict(C=9), dict(c=-1),
           dict(c=C), dict(d=0), dict(h=0), dict(w=-1), dict(a=ok["a"] + 2), dict(ws=ok["ws"] + 2), dict(ws=None, k=cnt.ptr() + 2),
           dict(b=(0, 0, 0, 13, 0, 19)), dict(b=(0, 6, 0, 13, 0, 19)), dict(b=(0, 5, 3, 2, 0, 19)), dict(b=(0, 5, 0, 13, -1, 19)),
           dict(b=(0, 5, 0, 13, 0, 20)), dict(tb=(0, 0, 1)), dict(tb=(0, 1, 3)), dict(f=8), dict(f=-1)]
    for kw in bad:
        assert rc(**kw) == -1, kw
    assert rc(d=2048, h=1024, w=1024, b=(0, 1, 0, 1, 0, 1)) == -2
    ws = g["dst"]
    assert bool((ws.buf[ws.off:ws.off + n] == FILL).all()) and _intact(g) and cnt.changed_anywhere() == 0
    assert rc(ws=None, k=cnt.ptr()) == 0                                                    # the other kind of weight


def test_wrapper():
    from boxsegliver_amd import ops
    acc, weight = _exact_inputs("cnt", seed=2)
    a, w = torch.from_numpy(acc).cuda(), torch.from_numpy(weight).cuda()
    _, want = iref.prob(acc, weight, 1)
    got = ops.eval3d_prob(a, w, 1)
    assert got.dtype == torch.uint8 and got.shape == (int(np.prod(VOL)),)
    np.testing.assert_array_equal(got.cpu().numpy(), iref.file_order(want, (2, 1, 0), (False,) * 3))
    _, want = iref.prob(acc, weight, 2, (1, 3, 0, 13, 2, 9))
    got = ops.eval3d_prob(a, w, 2, (1, 3, 0, 13, 2, 9), (1, 0, 2), (True, False, True))
    np.testing.assert_array_equal(got.cpu().numpy(), iref.file_order(want, (1, 0, 2), (True, False, True)))
    with pytest.raises(ValueError, match="permutation"):
        ops.eval3d_prob(a, w, 1, trans_bk=(1, 1, 2))
