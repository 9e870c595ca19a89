"""GPU: `unetk_eval3d_accumulate_w` and `unetk_eval3d_finish` (csrc/lits3d.hip) against their float64
restatement (eval3d_weighted_ref.py), and `liver_3d --mode eval --eval_in_patches` with `--eval_window_weight gaussian` and
with `--eval_box_from`, from the command line.  The shapes are those of test_gpu_eval3d.py."""
import ctypes

import numpy as np
import pytest
import torch

import eval3d_ref
import eval3d_weighted_ref as wref
import guardbuf
import lits3d_ref as ref

pytestmark = pytest.mark.gpu

SMALL = (6, 16, 20)
HW = (ref.H, ref.W)
ZOOMED = (18, 22)                    # int32((16, 20) * 1.125)
FLIPS = [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in range(8)]
SENTINEL = 0x7FBADBAD
ONES = tuple(np.ones(n, np.float32) for n in SMALL)


@pytest.fixture(scope="module")
def store():
    host = eval3d_ref.HostStore()
    host.cases = ref.make_cases()
    host.dev_im = torch.from_numpy(host.im.view(np.int16)).cuda()
    host.dev_lb = torch.from_numpy(host.lb).cuda()
    return host


def _case_rows(store, ci, crop):
    """As test_gpu_eval3d.py: the eight volume corners (one flip combination each), eight overlapping interior rows with all
    eight flips and a few shifted ones; the shallow case 2 gets rows that hang below its depth.  At most 5 rows go into a call."""
    depth = ref.DEPTHS[ci]
    mid = (depth // 2, 19, 23)
    corners = [(z, y, x) for z in (0, depth - 1) for y in (0, ref.H - 1) for x in (0, ref.W - 1)]
    centres = corners + [mid] * 8 + [(mid[0] - 1, 22, 25), (mid[0] + 1, 12, 30), (depth - 1, 39, 0)]
    return np.stack([ref.table_row(store.offset[ci], depth, c, crop, FLIPS[j % 8]) for j, c in enumerate(centres)])


def _gaussian():
    from boxsegliver_amd.data import lits3d
    return lits3d.window_weights(SMALL, 0.125)


def _dev(tables):
    return tuple(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda() for g in tables)


def _zeros(depth, c):
    return (torch.zeros((depth,) + HW + (c,), dtype=torch.float32, device="cuda"),
            torch.zeros((depth,) + HW, dtype=torch.float32, device="cuda"))


def _accumulate_w(store, ci, tab, probs, tables, acc=None, wsum=None, box=None, step=5):
    """The rows in calls of at most `step`, every call over the union box of ALL rows (a larger box visits more voxels,
    none of which a row of another call touches)."""
    from boxsegliver_amd import ops
    depth = ref.DEPTHS[ci]
    if acc is None:
        acc, wsum = _zeros(depth, probs.shape[-1])
    box = eval3d_ref.union_box(tab, SMALL, depth, HW) if box is None else box
    dtables = _dev(tables)
    for i in range(0, len(tab), step):
        ops.eval3d_accumulate_w(torch.from_numpy(np.ascontiguousarray(probs[i:i + step], dtype=np.float32)).cuda(),
                                torch.from_numpy(tab[i:i + step]).cuda(), SMALL, store.offset[ci], depth, box, dtables, acc, wsum,
                                store.dev_im, host_tab=tab[i:i + step])
    return acc, wsum


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------- (a) exact placement
@pytest.mark.parametrize("ci", [0, 2])
def test_zoom_one_rows_with_dyadic_tables_are_placed_bit_for_bit(store, ci):
    """crop = (H, W): every lerp fraction is 0, so a weight is a product of three table entries 2^-k, k <= 2; the
    probabilities are small integers: all sums are exact.  acc and wsum must equal the restatement bit for bit and nothing
    outside the union box may be touched.  All eight flips, the eight corners, overlapping rows, the shallow case."""
    depth = ref.DEPTHS[ci]
    tab = _case_rows(store, ci, SMALL[1:])
    rng = np.random.default_rng(5 + ci)
    tables = tuple((2.0 ** -rng.integers(0, 3, size=n)).astype(np.float32) for n in SMALL)
    for rows in (tab, tab[8:]):                                       # the whole case; a union box smaller than the case
        probs = rng.integers(0, 8, size=(len(rows),) + SMALL + (3,)).astype(np.float32)
        z0, z1, y0, y1, x0, x1 = box = eval3d_ref.union_box(rows, SMALL, depth, HW)
        assert (box == (0, depth, 0, ref.H, 0, ref.W)) == (rows is tab)
        want_acc = np.full((depth,) + HW + (3,), SENTINEL, np.int32).view(np.float32)
        want_w = np.full((depth,) + HW, SENTINEL, np.int32).view(np.float32)
        want_acc[z0:z1, y0:y1, x0:x1] = 0
        want_w[z0:z1, y0:y1, x0:x1] = 0
        acc, wsum = torch.from_numpy(want_acc.copy()).cuda(), torch.from_numpy(want_w.copy()).cuda()
        _accumulate_w(store, ci, rows, probs, tables, acc, wsum, box)
        s = wref.accumulate(rows, probs, tables, SMALL, depth, HW)
        racc, rw, hits = s.acc, s.wsum, s.hits
        assert hits.max() >= 8 and (ci != 2 or hits.sum() == len(rows) * depth * 16 * 20)
        assert np.array_equal(racc.astype(np.float32).astype(np.float64), racc) and np.array_equal(rw.astype(np.float32), rw)
        inside = np.zeros((depth,) + HW, bool)
        inside[z0:z1, y0:y1, x0:x1] = True
        want_acc[inside] = racc[inside].astype(np.float32)
        want_w[inside] = rw[inside].astype(np.float32)
        np.testing.assert_array_equal(_bits(wsum), want_w.view(np.int32))
        np.testing.assert_array_equal(_bits(acc), want_acc.view(np.int32))


# ------------------------------------------------------------------------------------------------- (b) ones tables
@pytest.mark.parametrize("ci", [0, 2])
def test_ones_tables_give_the_unweighted_kernel(store, ci):
    from boxsegliver_amd import ops
    depth = ref.DEPTHS[ci]
    tab = _case_rows(store, ci, ZOOMED)
    probs = np.random.default_rng(41 + ci).random((len(tab),) + SMALL + (3,), dtype=np.float32)
    box = eval3d_ref.union_box(tab, SMALL, depth, HW)
    acc, wsum = _accumulate_w(store, ci, tab, probs, ONES, box=box)
    pacc = torch.zeros_like(acc)
    cnt = torch.zeros((depth,) + HW, dtype=torch.int32, device="cuda")
    for i in range(0, len(tab), 5):
        ops.eval3d_accumulate(torch.from_numpy(probs[i:i + 5]).cuda(), torch.from_numpy(tab[i:i + 5]).cuda(), SMALL,
                              store.offset[ci], depth, box, pacc, cnt, store.dev_im, host_tab=tab[i:i + 5])
    assert int(cnt.max()) >= 8
    assert torch.equal(acc.view(torch.int32), pacc.view(torch.int32))
    assert torch.equal(wsum, cnt.to(torch.float32))


# ------------------------------------------------------------------------------------------------- (c) Gaussian tables
def test_gaussian_tables_on_zoomed_windows_match_the_restatement(store):
    """18 x 22 crops, all flips, C = 3, the tables of window_weights(SMALL, 0.125): per voxel and class
    |acc - ref| <= 2^-24 hits (K wmax max|probs| + |ref|) with K = 25, and |wsum - ref| <= 2^-24 hits (8 wmax + |ref|),
    against the restatement run in float64 with the SAME float32 tables.  K is counted in eval3d_weighted_ref.bound from
    the kernel's fp32 operations: 8 for the weight (two 3-operation lerps and two products), 16 for the bilerp of the
    probabilities (the constant of eval3d_ref.bound), 1 for their product.  wmax is per voxel, the largest weight any of
    its hits can have (the larger tap in place of each lerp), at most the tables' maximum 1: a voxel that only rims of
    windows reach is held to its own small weights."""
    tables = _gaussian()
    assert max(float(g.max()) for g in tables) == 1.0
    worst = worst_w = 0.0
    for ci in (0, 2):
        depth = ref.DEPTHS[ci]
        tab = _case_rows(store, ci, ZOOMED)
        probs = np.random.default_rng(17 + ci).random((len(tab),) + SMALL + (3,), dtype=np.float32)
        acc, wsum = _accumulate_w(store, ci, tab, probs, tables)
        s = wref.accumulate(tab, probs, tables, SMALL, depth, HW)
        racc, rw, hits = s.acc, s.wsum, s.hits
        assert hits.max() >= 8 and s.wmax.max() <= 1.0
        hit = hits > 0
        err = np.abs(acc.cpu().numpy().astype(np.float64) - racc)
        errw = np.abs(wsum.cpu().numpy().astype(np.float64) - rw)
        bound, boundw = wref.bound(s, np.abs(probs).max()), wref.bound_wsum(s)
        frac, fracw = float((err[hit] / bound[hit]).max()), float((errw[hit] / boundw[hit]).max())
        print("eval3d_accumulate_w case {}: max error / bound = {:.3f} (acc), {:.3f} (wsum)".format(ci, frac, fracw))
        worst, worst_w = max(worst, frac), max(worst_w, fracw)
        assert np.all(err <= bound), (ci, frac)
        assert np.all(errw <= boundw), (ci, fracw)
        assert np.all(err[~hit] == 0) and np.all(errw[~hit] == 0)
        assert np.all(wsum.cpu().numpy()[hit] > 0)
    print("eval3d_accumulate_w zoomed: worst error / bound = {:.3f} (acc), {:.3f} (wsum)".format(worst, worst_w))


# ------------------------------------------------------------------------------------------------- (d) order, guard bands
def test_order_split_calls_and_reproducibility(store):
    tab = _case_rows(store, 0, ZOOMED)[6:11]                          # two corners and three stacked rows, one call
    probs = np.random.default_rng(23).random((len(tab),) + SMALL + (3,), dtype=np.float32)
    tables = _gaussian()
    box = eval3d_ref.union_box(tab, SMALL, 12, HW)
    a = _accumulate_w(store, 0, tab, probs, tables, box=box)
    b = _accumulate_w(store, 0, tab, probs, tables, box=box)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    for k in (1, 3):                                                  # one call with [a; b] = a call with a, then one with b
        acc, wsum = _accumulate_w(store, 0, tab[:k], probs[:k], tables, box=box)
        _accumulate_w(store, 0, tab[k:], probs[k:], tables, acc, wsum, box=box)
        assert torch.equal(a[0].view(torch.int32), acc.view(torch.int32)) and torch.equal(a[1].view(torch.int32), wsum.view(torch.int32))
    perm = np.arange(len(tab))[::-1].copy()                           # the row order is part of the result
    c = _accumulate_w(store, 0, tab[perm], probs[perm], tables, box=box)
    assert not torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))


def _guarded_call(store, ci, rows):
    """Everything the entry point sees inside guard bands -> (call, dict of the guarded buffers, box, want)."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    depth = ref.DEPTHS[ci]
    tab = _case_rows(store, ci, ZOOMED)[rows]
    n = len(tab)
    probs = np.random.default_rng(29).random((n,) + SMALL + (3,), dtype=np.float32)
    tables = _gaussian()
    box = eval3d_ref.union_box(tab, SMALL, depth, HW)
    want = _accumulate_w(store, ci, tab, probs, tables)
    g = dict(acc=guardbuf.guarded((depth,) + HW + (3,)), wsum=guardbuf.guarded((depth,) + HW + (1,)))
    for out in g.values():
        out.view.zero_()
        out.snap = out.flat.clone()
    g["probs"] = guardbuf.guarded_input(torch.from_numpy(probs).cuda())
    g["tab"] = guardbuf.guarded_input(torch.from_numpy(tab).cuda().view(torch.float32))
    for name, t in zip(("gz", "gy", "gx"), _dev(tables)):
        g[name] = guardbuf.guarded_input(t.view(-1, 1))
    desc = ops.lits3d_desc(store.dev_im, n, SMALL, False)
    cbox = (ctypes.c_int32 * 6)(*box)
    default = dict(d=desc, t=g["tab"].ptr(), p=g["probs"].ptr(), c=3, base=store.offset[ci], dep=depth, b=cbox, gz=g["gz"].ptr(),
                   gy=g["gy"].ptr(), gx=g["gx"].ptr(), a=g["acc"].ptr(), w=g["wsum"].ptr())

    def call(**kw):
        v = dict(default, **kw)
        P = ctypes.c_void_p
        return lib.unetk_eval3d_accumulate_w(ctypes.byref(v["d"]), P(v["t"]), P(v["p"]), v["c"], v["base"], v["dep"], v["b"], P(v["gz"]),
                                             P(v["gy"]), P(v["gx"]), P(v["a"]), P(v["w"]), _abi.stream_ptr())
    call.default = default
    return call, g, box, want


def test_guard_bands_around_every_buffer(store):
    """The shallow case: windows hang below the volume.  acc, wsum, probs, the table and the three weight tables sit in
    guard bands; the outputs equal an unguarded call, nothing else changes."""
    call, g, _, want = _guarded_call(store, 2, slice(6, 11))
    assert call() == 0
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check_untouched(), name
        if name not in ("acc", "wsum"):
            assert buf.changed_anywhere() == 0, name
    assert torch.equal(g["acc"].view.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(g["wsum"].view.view(torch.int32)[..., 0], want[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------- (g) arguments
def test_accumulate_w_rejects_bad_arguments_before_it_writes(store):
    from boxsegliver_amd import _abi, ops
    ci, depth = 2, ref.DEPTHS[2]
    call, g, box, want = _guarded_call(store, ci, slice(6, 11))
    big = ops.lits3d_desc(store.dev_im, 5, (2048, 1024, 1024), False)
    assert call(d=big) == -2                                                          # UNETK_E_UNSUPPORTED, as unetk_lits_patch3d
    wide = ops.lits3d_desc(store.dev_im, 5, (1024, 1024, 1024), False)               # D H W < 2^31 <= D H W C
    assert call(d=wide, c=3) == -2
    for name in ("p", "t", "a", "w", "b", "gz", "gy", "gx"):
        assert call(**{name: None}) == -1, name
    for name in ("p", "t", "a", "w", "gz", "gy", "gx"):                               # 2 bytes off a float / int32 boundary
        assert call(**{name: call.default[name] + 2}) == -1, name
    assert call(c=0) == -1 and call(c=9) == -1
    for bad in ((0, depth + 1, 0, 40, 0, 48), (-1, depth, 0, 40, 0, 48), (0, depth, 0, 41, 0, 48), (0, depth, 0, 40, 0, 49),
                (0, depth, 5, 5, 0, 48), (0, depth, 0, 40, 9, 3)):
        assert call(b=(ctypes.c_int32 * 6)(*bad)) == -1, bad
    assert call(dep=0) == -1 and call(base=-1) == -1 and call(base=store.im.shape[0]) == -1
    bad_desc = ops.lits3d_desc(store.dev_im, 0, SMALL, False)
    assert call(d=bad_desc) == -1
    torch.cuda.synchronize()
    assert all(buf.changed_anywhere() == 0 for buf in g.values())
    # a row of another case contributes nothing on the device; the wrapper, which has the host table, refuses it
    assert call(base=store.offset[3], dep=depth) == 0 and call(dep=depth - 1, b=(ctypes.c_int32 * 6)(0, depth - 1, 0, 40, 0, 48)) == 0
    torch.cuda.synchronize()
    assert all(buf.changed_anywhere() == 0 for buf in g.values())
    tab = _case_rows(store, ci, ZOOMED)[6:11]
    probs = torch.zeros((5,) + SMALL + (3,), device="cuda")
    acc, wsum = _zeros(depth, 3)
    tables = _dev(_gaussian())
    foreign = tab.copy()
    foreign[3, 0] = store.offset[3]
    with pytest.raises(_abi.UnetkError, match="base, depth"):
        ops.eval3d_accumulate_w(probs, torch.from_numpy(foreign).cuda(), SMALL, store.offset[ci], depth, box, tables, acc, wsum,
                                store.dev_im, host_tab=foreign)
    with pytest.raises(_abi.UnetkError, match="device tensors"):
        ops.eval3d_accumulate_w(probs, torch.from_numpy(tab).cuda(), SMALL, store.offset[ci], depth, box,
                                tuple(t.cpu() for t in tables), acc, wsum, store.dev_im)
    with pytest.raises(AssertionError):                                               # an int32 count is not a weight volume
        ops.eval3d_accumulate_w(probs, torch.from_numpy(tab).cuda(), SMALL, store.offset[ci], depth, box, tables, acc,
                                wsum.to(torch.int32), store.dev_im)
    with pytest.raises(AssertionError):                                               # a table of another length
        ops.eval3d_accumulate_w(probs, torch.from_numpy(tab).cuda(), SMALL, store.offset[ci], depth, box,
                                (tables[0], tables[2], tables[1]), acc, wsum, store.dev_im)
    assert float(acc.abs().max()) == 0 and float(wsum.abs().max()) == 0


def test_finish_rejects_bad_arguments_before_it_writes():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    vol = (5,) + HW
    acc = guardbuf.guarded_input(torch.rand(vol + (3,), device="cuda"))
    wsum = guardbuf.guarded_input(torch.ones(vol + (1,), device="cuda"))
    cnt = guardbuf.guarded_input(torch.ones(vol + (1,), dtype=torch.int32, device="cuda").view(torch.float32))
    pred = torch.full(vol, 77, dtype=torch.uint8, device="cuda")
    unc = guardbuf.guarded((1, 1))
    unc.view.view(torch.int32).zero_()
    unc.snap = unc.flat.clone()
    default = dict(a=acc.ptr(), c=3, d=5, h=ref.H, w=ref.W, ws=wsum.ptr(), k=None, b=(ctypes.c_int32 * 6)(0, 5, 0, ref.H, 0, ref.W),
                   p=pred.data_ptr(), u=unc.ptr())

    def call(**kw):
        v = dict(default, **kw)
        P = ctypes.c_void_p
        return lib.unetk_eval3d_finish(P(v["a"]), v["c"], v["d"], v["h"], v["w"], P(v["ws"]), P(v["k"]), v["b"], P(v["p"]), P(v["u"]),
                                       _abi.stream_ptr())
    assert call(a=None) == -1 and call(p=None) == -1 and call(u=None) == -1 and call(b=None) == -1
    assert call(ws=None) == -1 and call(k=cnt.ptr()) == -1                            # neither weight; both
    assert call(c=0) == -1 and call(c=9) == -1 and call(d=0) == -1 and call(h=0) == -1 and call(w=-1) == -1
    assert call(a=acc.ptr() + 2) == -1 and call(ws=wsum.ptr() + 2) == -1 and call(ws=None, k=cnt.ptr() + 2) == -1
    assert call(u=unc.ptr() + 2) == -1
    for bad in ((0, 6, 0, 40, 0, 48), (-1, 5, 0, 40, 0, 48), (0, 5, 0, 41, 0, 48), (0, 5, 0, 40, 0, 49), (0, 5, 5, 5, 0, 48),
                (0, 5, 0, 40, 9, 3), (3, 2, 0, 40, 0, 48)):
        assert call(b=(ctypes.c_int32 * 6)(*bad)) == -1, bad
    assert call(d=2048, h=1024, w=1024, b=(ctypes.c_int32 * 6)(0, 5, 0, 40, 0, 48)) == -2   # depth src_h src_w >= 2^31
    torch.cuda.synchronize()
    assert int((pred != 77).sum()) == 0 and unc.changed_anywhere() == 0
    assert acc.changed_anywhere() == 0 and wsum.changed_anywhere() == 0 and cnt.changed_anywhere() == 0
    # and the call itself, with either weight
    for kw in (dict(), dict(ws=None, k=cnt.ptr())):
        assert call(**kw) == 0
        torch.cuda.synchronize()
        assert unc.changed_anywhere() == 0 and unc.check_untouched()
        np.testing.assert_array_equal(pred.cpu().numpy(), np.argmax(acc.view.cpu().numpy(), axis=-1))
        pred.fill_(77)
    assert acc.changed_anywhere() == 0 and wsum.changed_anywhere() == 0 and cnt.changed_anywhere() == 0


# ------------------------------------------------------------------------------------------------- (e) the finishing step
@pytest.mark.parametrize("kind", ["wsum", "cnt"])
def test_finish_is_head_predict_where_covered_and_counts_the_holes(kind):
    from boxsegliver_amd import ops
    vol = (9,) + HW
    rng = np.random.default_rng(31)
    acc_h = rng.integers(0, 3, size=vol + (3,)).astype(np.float32)                  # many ties: the lowest index must win
    acc = torch.from_numpy(acc_h).cuda()
    dtype = torch.float32 if kind == "wsum" else torch.int32
    weight_h = rng.integers(1, 5, size=vol)
    if kind == "wsum":
        weight_h = weight_h * 2.0 ** -40                                             # small weights are weights
    whole = (0, 9, 0, ref.H, 0, ref.W)
    amax, _ = ops.head_predict(acc.view(-1, 3), 3, want_preds=False)
    amax = amax.view(vol).cpu().numpy()
    assert len(np.unique(amax)) == 3 and np.array_equal(amax, np.argmax(acc_h, -1))

    def run(weight_h, box):
        unc = torch.zeros(1, dtype=torch.int32, device="cuda")
        pred = ops.eval3d_finish(acc, torch.from_numpy(np.ascontiguousarray(weight_h)).to(dtype).cuda(), box, unc)
        assert pred.dtype == torch.uint8 and tuple(pred.shape) == vol
        return pred.cpu().numpy(), int(unc.item())
    pred, unc = run(weight_h, whole)                                                 # fully covered: head_predict everywhere
    np.testing.assert_array_equal(pred, amax)
    assert unc == 0
    # a hole that straddles the box: rows of full waves, parts of waves, single voxels; zero and (cnt) negative weights
    holed = weight_h.copy()
    holed[2:5, 7:30, 3:41] = 0
    holed[6, 20, 17] = 0
    holed[8, 39, 47] = 0 if kind == "wsum" else -3
    holed[0, 0, 0] = 0
    box = (1, 9, 10, 40, 5, 48)
    want, want_unc = wref.finish(acc_h, holed, box)
    assert want_unc == 3 * 20 * 36 + 2 and (holed <= 0).sum() > want_unc              # holes outside the box are not counted
    first = run(holed, box)
    np.testing.assert_array_equal(first[0], want)
    assert first[1] == want_unc
    second = run(holed, box)
    assert second[1] == first[1] and np.array_equal(second[0], first[0])
    assert first[0][holed <= 0].max() == 0 and first[0][0].max() == 0 and first[0][:, :10].max() == 0
    inside = np.zeros(vol, bool)
    inside[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
    np.testing.assert_array_equal(first[0][inside & (holed > 0)], amax[inside & (holed > 0)])


# ------------------------------------------------------------------------------------------------- (f) round trip
def test_round_trip_with_the_patch_kernel_and_gaussian_weights(store):
    """Windows of the plan cut over case 0 by unetk_lits_patch3d, probs = one-hot of the window's labels scaled to
    {0.75, 0.125, 0.125}, accumulated with the Gaussian tables and finished: equal to the same pipeline in the restatement at
    EVERY voxel.  The restatement's smallest top-two gap is asserted to exceed twice the bound of
    test_gaussian_tables_on_zoomed_windows_match_the_restatement (either sum may move by it); on the CPU, with the
    restatement alone, the smallest gap / bound over the case is 114.3."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits3d
    ci, depth = 0, ref.DEPTHS[0]
    im, lb = store.cases[ci]
    tables = _gaussian()
    dtables = _dev(tables)
    acc, wsum = _zeros(depth, 3)
    s = None
    plan = list(lits3d.eval_tables(store.meta[ci], store, SMALL, 0.5, FLIPS, 32))
    for tab in plan:
        dtab = torch.from_numpy(tab).cuda()
        _, labels = ops.lits_patch3d(store.dev_im, store.dev_lb, dtab, SMALL, False, 2)
        want_lab = np.stack([ref.patch(im, lb, r[2:5], r[5:7], SMALL, tuple(r[7:10]))[1] for r in tab])
        np.testing.assert_array_equal(labels.cpu().numpy(), want_lab)
        probs = torch.full(labels.shape + (3,), 0.125, dtype=torch.float32, device="cuda")
        probs.scatter_(-1, labels.long().unsqueeze(-1), 0.75)
        ops.eval3d_accumulate_w(probs, dtab, SMALL, store.offset[ci], depth, lits3d.table_box(tab, SMALL, depth, HW), dtables, acc,
                                wsum, store.dev_im, host_tab=tab)
        rprobs = np.full(want_lab.shape + (3,), 0.125)
        np.put_along_axis(rprobs, want_lab[..., None], 0.75, axis=-1)
        s = wref.accumulate(tab, rprobs, tables, SMALL, depth, HW, s)
    racc = s.acc
    assert len(plan) == 12 and s.hits.min() >= 8
    gap = eval3d_ref.top_two_gap(racc)
    bound = wref.bound(s, 0.75).max(axis=-1)
    print("weighted round trip: smallest top-two gap / bound = {:.1f}".format(float((gap / bound).min())))
    assert np.all(gap > 2 * bound)
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.eval3d_finish(acc, wsum, (0, depth, 0, ref.H, 0, ref.W), unc).cpu().numpy()
    assert int(unc.item()) == 0
    np.testing.assert_array_equal(got, np.argmax(racc, axis=-1))
    assert {int(v) for v in np.unique(got)} == {0, 1, 2}
    assert (got == lb).mean() > 0.97


# ------------------------------------------------------------------------------------------------- (h) end to end
def test_liver_3d_evaluates_with_gaussian_windows_and_inside_a_box(tmp_path, monkeypatch):
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits3d
    from boxsegliver_amd.entry import main as entry
    cases = ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = ("liver_3d --mode train --tag cli3dw --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 4 --batches_per_epoch 2 --evaluator Volume --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --log_step 1").split()
    argv += ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    assert entry.main(argv) == 0
    ev = list(argv)
    ev[ev.index("--mode") + 1] = "eval"
    ev[ev.index("--batch_size") + 1] = "8"
    ev += "--eval_in_patches --eval_final".split()
    shape = (4, 32, 32)
    keys = [(0, ref.DEPTHS[2]), (ref.DEPTHS[2], ref.DEPTHS[3])]                       # (base, depth) of the validation cases 2, 3
    real = {name: getattr(ops, name) for name in ("eval3d_accumulate", "eval3d_accumulate_w", "eval3d_finish", "head_predict")}
    records, volumes = [], []

    def recording_acc(probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=None):
        records.append((sample_tab.cpu().numpy(), probs.cpu().numpy(), int(case_base), int(case_depth), tuple(box), None))
        return real["eval3d_accumulate"](probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=host_tab)

    def recording_acc_w(probs, sample_tab, shape, case_base, case_depth, box, tables, acc, wsum, slices, host_tab=None):
        records.append((sample_tab.cpu().numpy(), probs.cpu().numpy(), int(case_base), int(case_depth), tuple(box),
                        tuple(t.cpu().numpy() for t in tables)))
        return real["eval3d_accumulate_w"](probs, sample_tab, shape, case_base, case_depth, box, tables, acc, wsum, slices,
                                           host_tab=host_tab)

    def recording_finish(acc, weight, box, uncovered):
        out = real["eval3d_finish"](acc, weight, box, uncovered)
        volumes.append((out.cpu().numpy(), tuple(box), weight.dtype))
        return out

    def recording_predict(probs, ncls, want_preds=True):
        out = real["head_predict"](probs, ncls, want_preds)
        if not want_preds:
            volumes.append((out[0].cpu().numpy(), None, None))
        return out

    def evaluate(extra):
        del records[:], volumes[:]
        monkeypatch.setattr(ops, "eval3d_accumulate", recording_acc)
        monkeypatch.setattr(ops, "eval3d_accumulate_w", recording_acc_w)
        monkeypatch.setattr(ops, "eval3d_finish", recording_finish)
        monkeypatch.setattr(ops, "head_predict", recording_predict)
        args, sub, pipe = entry.get_arguments(ev + extra)
        results = entry.run(args, sub, pipe)
        monkeypatch.undo()
        per_case = {}
        for tab, probs, base, depth, box, tables in records:
            assert len(tab) <= 8 and (tab[:, 0] == base).all() and (tab[:, 1] == depth).all()
            assert box == eval3d_ref.union_box(tab, shape, depth, HW)
            per_case.setdefault((base, depth), []).append((tab, probs, tables))
        assert sorted(per_case) == keys and len(volumes) == 2
        return per_case, list(volumes), results

    # ---- Gaussian windows, all eight mirrors
    per_case, vols, results = evaluate("--eval_window_weight gaussian --eval_mirror --random_flip 7".split())
    for key in ("Liver/Dice", "Tumor/Dice", "GLiverDice", "GTumorDice"):
        assert np.isfinite(results[key]) and 0.0 <= results[key] <= 1.0, (key, results)
    want_tables = lits3d.window_weights(shape, 0.125)
    total = excluded = 0
    for (base, depth), (got, box, wdtype) in zip(keys, vols):
        assert box == (0, depth, 0, ref.H, 0, ref.W) and wdtype == torch.float32
        s = None
        max_prob = 0.0
        for tab, probs, tables in per_case[(base, depth)]:
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(tables, want_tables))
            s = wref.accumulate(tab, probs, tables, shape, depth, HW, s)
            max_prob = max(max_prob, float(np.abs(probs).max()))
            assert set(map(tuple, tab[:, 7:10])) == set(FLIPS)
        assert s.hits.min() >= 8 and s.wsum.min() > 0
        sure = eval3d_ref.top_two_gap(s.acc) > 2 * wref.bound(s, max_prob).max(axis=-1)   # either sum may move by the bound
        want = np.argmax(s.acc, axis=-1)
        np.testing.assert_array_equal(got[sure], want[sure])
        total += sure.size
        excluded += int((~sure).sum())
    print("liver_3d eval, gaussian: {} of {} voxels excluded (top-two gap within the rounding bound)".format(excluded, total))
    assert excluded <= 0.01 * total

    # ---- no new flag: the calls of the plain path and nothing else; its volumes are those calls made by hand
    per_case, vols, plain_results = evaluate([])
    plain_rows = {k: sum(len(t) for t, _, _ in v) for k, v in per_case.items()}
    for (base, depth), (got, box, _) in zip(keys, vols):
        assert box is None                                                            # head_predict, not eval3d_finish
        acc = torch.zeros((depth,) + HW + (3,), dtype=torch.float32, device="cuda")
        cnt = torch.zeros((depth,) + HW, dtype=torch.int32, device="cuda")
        slices = torch.zeros((ref.DEPTHS[2] + ref.DEPTHS[3],) + HW, dtype=torch.int16, device="cuda")   # its extent is all that enters
        for tab, probs, tables in per_case[(base, depth)]:
            assert tables is None                                                     # eval3d_accumulate, not _w
            ops.eval3d_accumulate(torch.from_numpy(probs).cuda(), torch.from_numpy(tab).cuda(), shape, base, depth,
                                  lits3d.table_box(tab, shape, depth, HW), acc, cnt, slices, host_tab=tab)
        assert int(cnt.min()) > 0
        amax, _ = ops.head_predict(acc.view(-1, 3), 3, want_preds=False)
        np.testing.assert_array_equal(got.reshape(-1), amax.cpu().numpy())

    # ---- windows restricted to the box of a saved prediction (here: the cases' own foreground)
    coarse = tmp_path / "coarse"
    coarse.mkdir()
    for pid in (2, 3):
        wref.write_prediction(coarse, pid, cases[pid][1])
    per_case, vols, boxed_results = evaluate(["--eval_box_from", str(coarse), "--eval_box_margin", "0", "2", "2"])
    total = excluded = 0
    for pid, (base, depth), (got, box, wdtype) in zip((2, 3), keys, vols):
        assert box == lits3d.prediction_box(coarse, pid, depth, HW, (0, 2, 2)) == (1, depth - 1, 4, 37, 4, 41)
        assert wdtype == torch.int32
        rows = sum(len(t) for t, _, _ in per_case[(base, depth)])
        assert rows < plain_rows[(base, depth)]                                       # fewer windows were served
        racc = rcnt = None
        max_prob = 0.0
        for tab, probs, tables in per_case[(base, depth)]:
            assert tables is None
            racc, rcnt = eval3d_ref.accumulate(tab, probs, shape, depth, HW, racc, rcnt)
            max_prob = max(max_prob, float(np.abs(probs).max()))
        inside = np.zeros((depth,) + HW, bool)
        inside[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
        assert rcnt[inside].min() >= 1 and (rcnt[~inside] > 0).any()                  # windows reach beyond the box ...
        assert got[~inside].max() == 0                                                # ... and leave no prediction there
        sure = inside & (eval3d_ref.top_two_gap(racc) > 2 * eval3d_ref.bound(racc, rcnt, max_prob).max(axis=-1))
        np.testing.assert_array_equal(got[sure], np.argmax(racc, axis=-1)[sure])
        total += int(inside.sum())
        excluded += int((inside & ~sure).sum())
    print("liver_3d eval, boxed: {} of {} voxels excluded".format(excluded, total))
    assert excluded <= 0.01 * total
    for key in ("Liver/Dice", "GLiverDice"):
        assert np.isfinite(boxed_results[key]) and 0.0 <= boxed_results[key] <= 1.0
    # a coarse prediction that misses a case is an error, not a whole-volume run
    (coarse / "predict-3.nii.gz").unlink()
    with pytest.raises(FileNotFoundError, match="predict-3.nii.gz"):
        entry.main(ev + ["--eval_box_from", str(coarse)])
