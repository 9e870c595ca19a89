"""GPU: the z-resampling kernels of --z_spacing (csrc/lits3d.hip): `unetk_lits_patch3d_z` against its
restatement (lits3d_zspace_ref.py) and, for rows whose crop depth equals D, against `unetk_lits_patch3d` bit for bit;
`unetk_eval3d_accumulate_z` / `_wz` against theirs and, with every crop depth D, against `unetk_eval3d_accumulate` / `_w`."""
import ctypes

import numpy as np
import pytest
import torch

import eval3d_ref
import guardbuf
import lits3d_ref as ref
import lits3d_zspace_ref as zref

pytestmark = pytest.mark.gpu

SHAPE, FLAT = (4, 12, 10), (1, 8, 8)           # FLAT: D == 1 makes zs = 0
HW = (ref.H, ref.W)
FLIPS = [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in range(8)]
NORMAL, SHALLOW = 0, 2                         # lits3d_ref cases: 12 slices, 5 slices
ZMAX = 1 << 10


@pytest.fixture(scope="module")
def store():
    host = eval3d_ref.HostStore()
    host.cases = ref.make_cases()
    host.dev_im = torch.from_numpy(host.im.view(np.int16)).cuda()
    host.dev_lb = torch.from_numpy(host.lb).cuda()
    return host


def _depths(shape, ci):
    """The crop depths of the issue for a D-deep patch of case ci: 1, D, 2D + 1, D - 1 (0 is clamped to 1), depth + 3."""
    d = shape[0]
    return [1, d, 2 * d + 1, d - 1, ref.DEPTHS[ci] + 3]


def _crop(shape, zoom):
    from boxsegliver_amd.data import lits3d
    return tuple(int(v) for v in lits3d.crop_shape(shape[1:], [zoom, zoom * 0.97 + 0.03]))


def _samples(shape, zoom):
    """(case, centre, crop, flips, zcrop): every crop depth on the normal and on the shallow case under all eight flips;
    the centres walk through the case, its first and last slice included."""
    crop = _crop(shape, zoom)
    out = []
    for ci, centres in ((NORMAL, [(0, 0, 0), (6, 19, 23), (11, 39, 47), (3, 25, 8)]), (SHALLOW, [(2, 17, 21), (4, 39, 0), (0, 5, 44)])):
        for k, cd in enumerate(_depths(shape, ci)):
            out += [(ci, centres[(k + j) % len(centres)], crop, f, cd) for j, f in enumerate(FLIPS)]
    return out


def _table(store, samples, gammas=None):
    rows = [ref.table_row(store.offset[ci], ref.DEPTHS[ci], c, crop, flips, 1.0 if gammas is None else gammas[j])
            for j, (ci, c, crop, flips, _) in enumerate(samples)]
    return np.stack(rows)


def _zcrop(samples):
    return np.array([s[4] for s in samples], dtype=np.int32)


def _run(store, tab, zcrop, shape, training=False, lab_max=2, zmax=ZMAX):
    from boxsegliver_amd import ops
    return ops.lits_patch3d(store.dev_im, store.dev_lb, torch.from_numpy(tab).cuda(), shape, training, lab_max,
                            zcrop=torch.from_numpy(np.asarray(zcrop, dtype=np.int32)).cuda(), zcrop_max=zmax)


def _check_against_restatement(store, samples, got, lab, lab1, shape, zmax=ZMAX):
    worst = 0.0
    for j, (ci, c, crop, flips, cd) in enumerate(samples):
        im, lb = store.cases[ci]
        want, want_lab, m, s = zref.patch(im, lb, c, crop, shape, cd, zmax, flips)
        np.testing.assert_array_equal(lab[j], want_lab, err_msg=str(samples[j]))
        if lab1 is not None:
            np.testing.assert_array_equal(lab1[j], np.minimum(want_lab, 1), err_msg=str(samples[j]))
        assert s > 0
        bound = 2.0 ** -24 * (abs(m) / s + 24 * max(1.0, np.abs(want).max()))
        err = np.abs(got[j].astype(np.float64) - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (samples[j], err, bound)
    return worst


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape,zoom", [(SHAPE, 1.0), (SHAPE, 1.4), (FLAT, 1.0), (FLAT, 1.4)])
def test_patch_z_matches_restatement(store, shape, zoom):
    """Labels exact (lab_max 2 and 1); images (no gamma) within 2^-24 (|m| / s + 24 max(1, max |ref|)): the bound of
    test_gpu_lits3d.py::test_patch_matches_restatement with 16 raised to 24 for the fourth lerp and its fraction."""
    samples = _samples(shape, zoom)
    tab, zc = _table(store, samples), _zcrop(samples)
    images, labels = _run(store, tab, zc, shape)
    assert images.shape == (len(samples),) + shape + (1,) and labels.shape == (len(samples),) + shape
    lab1 = _run(store, tab, zc, shape, lab_max=1)[1].cpu().numpy()
    lab = labels.cpu().numpy()
    worst = _check_against_restatement(store, samples, images[..., 0].cpu().numpy(), lab, lab1, shape)
    print("lits_patch3d_z {} zoom {}: max error / bound = {:.3f}".format(shape, zoom, worst))
    assert {int(v) for v in np.unique(lab)} == {0, 1, 2}


# ------------------------------------------------------------------------------------------------- cd == D
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("shape", [SHAPE, FLAT])
def test_rows_with_the_output_depth_equal_the_plain_entry_bit_for_bit(store, shape, training):
    """zcrop[n] == D: zs == 1, fz == 0 -- the row of unetk_lits_patch3d, bit for bit, gamma included; in a batch of such rows
    and in one that mixes them with resampled rows."""
    from boxsegliver_amd import ops
    samples = _samples(shape, 1.4)
    gammas = [0.7 + 0.01 * j for j in range(len(samples))]
    tab = _table(store, samples, gammas)
    plain = ops.lits_patch3d(store.dev_im, store.dev_lb, torch.from_numpy(tab).cuda(), shape, training)
    mixed_zc = _zcrop(samples)
    same = mixed_zc == shape[0]
    assert same.any() and (shape[0] == 1 or not same.all())
    for zc in (np.full(len(samples), shape[0], np.int32), mixed_zc):
        got = _run(store, tab, zc, shape, training)
        rows = torch.from_numpy(np.flatnonzero(zc == shape[0])).cuda()
        assert torch.equal(got[0][rows].view(torch.int32), plain[0][rows].view(torch.int32))
        assert torch.equal(got[1][rows], plain[1][rows])
    other = torch.from_numpy(np.flatnonzero(mixed_zc > shape[0])).cuda()
    assert not torch.equal(got[0][other], plain[0][other])                           # the resampled rows are other patches


# ------------------------------------------------------------------------------------------------- the shallow case
def test_slices_beyond_a_shallow_case_are_zeros(store):
    """Case 2 has 5 slices; a crop of 8 on a 4-slice patch samples crop slices 0, 7/3, 14/3, 7: output slice 3 lies beyond the
    case -- zeros, label 0 -- and slice 2 lerps the case's last slice (4) with the zero slice 5 at fz = 2/3: a third of the
    last slice's in-plane value, as the restatement gives it.  The front/back flip puts them at the other end."""
    crop = _crop(SHAPE, 1.0)
    samples = [(SHALLOW, (2, 17, 21), crop, (0, 0, 0), 8), (SHALLOW, (2, 17, 21), crop, (1, 0, 1), 8)]
    tab, zc = _table(store, samples), _zcrop(samples)
    images, labels = _run(store, tab, zc, SHAPE)
    got, lab = images[..., 0].cpu().numpy(), labels.cpu().numpy()
    _check_against_restatement(store, samples, got, lab, None, SHAPE)
    assert np.all(got[0][3] == 0) and np.all(lab[0][3] == 0) and np.all(got[1][0] == 0) and np.all(lab[1][0] == 0)
    im, lb = store.cases[SHALLOW]
    box = zref.crop_box((2, 17, 21), crop, 8, 5, HW)
    assert box[0] == 0
    planes = ref.resize_bilinear(ref.zscore(ref.crop(im, lb, box, 8)[0])[0], SHAPE[1:])
    assert np.all(planes[5:] == 0) and np.abs(planes[4]).max() > 0
    f = float(np.float32(2) * np.float32(7 / 3) - np.float32(4))
    assert abs(f - 2 / 3) < 1e-6
    np.testing.assert_allclose(got[0][2], (1 - f) * planes[4], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(got[1][1], got[0][2][:, ::-1])
    assert np.abs(got[0][2]).max() > 0 and np.all(lab[0][2] == 0)                     # nearest slice of 14/3 is 5: beyond the case


# ------------------------------------------------------------------------------------------------- bad inputs
def test_crop_depths_are_clamped_and_bad_arguments_rejected(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    crop = _crop(SHAPE, 1.4)
    samples = [(ci, c, crop, f, cd) for (ci, c, f), cd in zip([(NORMAL, (6, 19, 23), (0, 0, 0)), (SHALLOW, (2, 17, 21), (1, 1, 1)),
                                                               (NORMAL, (11, 3, 40), (0, 1, 0)), (NORMAL, (1, 30, 9), (1, 0, 1))],
                                                              (0, -5, 10 ** 6, 3))]
    tab, zc = _table(store, samples), _zcrop(samples)
    zmax = 9
    images, labels = _run(store, tab, zc, SHAPE, zmax=zmax)
    clamped = [(ci, c, cr, f, zref.clamp_cd(cd, zmax)) for ci, c, cr, f, cd in samples]
    assert [s[4] for s in clamped] == [1, 1, 9, 3]
    _check_against_restatement(store, clamped, images[..., 0].cpu().numpy(), labels.cpu().numpy(), None, SHAPE, zmax)
    again = _run(store, tab, _zcrop(clamped), SHAPE, zmax=zmax)
    assert torch.equal(images.view(torch.int32), again[0].view(torch.int32)) and torch.equal(labels, again[1])
    # the entry point's own checks
    n = len(samples)
    dtab, dz = torch.from_numpy(tab).cuda(), torch.from_numpy(np.concatenate([zc, zc])).cuda()
    desc = ops.lits3d_desc(store.dev_im, n, SHAPE, False)
    nbytes = int(lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(desc)))
    out_im = guardbuf.guarded((n,) + SHAPE + (1,))
    out_lb = guardbuf.guarded((n,) + SHAPE + (1,))
    ws = guardbuf.GuardedWorkspace(nbytes)

    def call(z=dz.data_ptr(), zmax=zmax, ws_bytes=nbytes):
        return lib.unetk_lits_patch3d_z(ctypes.byref(desc), _abi.ptr(store.dev_im), _abi.ptr(store.dev_lb), _abi.ptr(dtab),
                                        ctypes.c_void_p(z), zmax, ctypes.c_void_p(out_im.ptr()), ctypes.c_void_p(out_lb.ptr()),
                                        ctypes.c_void_p(ws.ptr()), ws_bytes, _abi.stream_ptr())
    limit = -(-(1 << 31) // (ref.H * ref.W))                       # the first zcrop_max with zcrop_max * src_h * src_w >= 2^31
    assert call(zmax=limit) == -2 and call(zmax=1 << 30) == -2     # UNETK_E_UNSUPPORTED
    assert call(z=None) == -1 and call(z=dz.data_ptr() + 2) == -1 and call(zmax=0) == -1       # UNETK_E_BADARG
    assert call(ws_bytes=nbytes - 1) == -3
    torch.cuda.synchronize()
    assert out_im.changed_anywhere() == 0 and out_lb.changed_anywhere() == 0          # nothing was launched
    assert call(z=dz.data_ptr() + 4 * n) == 0                      # aligned to 4 bytes, no more
    assert call(zmax=limit - 1) == 0                               # the largest supported bound: the entries stay what they are
    torch.cuda.synchronize()
    assert torch.equal(out_im.view.view(torch.int32), _run(store, tab, zc, SHAPE, zmax=limit - 1)[0].view(torch.int32))
    with pytest.raises(_abi.UnetkError, match="31-bit"):
        _run(store, tab, zc, SHAPE, zmax=limit)
    with pytest.raises(ValueError, match="rotate or warp"):
        ops.lits_patch3d(store.dev_im, store.dev_lb, dtab, SHAPE, False, rotate=True, zcrop=dz[:n], zcrop_max=zmax)


# ------------------------------------------------------------------------------------------------- bits and guards
@pytest.mark.parametrize("training", [False, True])
def test_two_calls_give_identical_bits_inside_guard_bands(store, training):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    samples = _samples(SHAPE, 1.4)
    n = len(samples)
    tab, zc = _table(store, samples, [0.7 + 0.01 * j for j in range(n)]), _zcrop(samples)
    a, b = _run(store, tab, zc, SHAPE, training), _run(store, tab, zc, SHAPE, training)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0]).all())
    desc = ops.lits3d_desc(store.dev_im, n, SHAPE, training)
    nbytes = int(lib.unetk_lits_patch3d_ws_bytes(ctypes.byref(desc)))
    images, labels = guardbuf.guarded((n,) + SHAPE + (1,)), guardbuf.guarded((n,) + SHAPE + (1,))
    ws = guardbuf.GuardedWorkspace(nbytes)
    gtab = guardbuf.guarded_input(torch.from_numpy(tab.view(np.float32)).cuda())
    gz = guardbuf.guarded_input(torch.from_numpy(zc.view(np.float32)[:, None]).cuda())
    assert lib.unetk_lits_patch3d_z(ctypes.byref(desc), _abi.ptr(store.dev_im), _abi.ptr(store.dev_lb), ctypes.c_void_p(gtab.ptr()),
                                    ctypes.c_void_p(gz.ptr()), ZMAX, ctypes.c_void_p(images.ptr()), ctypes.c_void_p(labels.ptr()),
                                    ctypes.c_void_p(ws.ptr()), nbytes, _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert images.check_untouched() and images.unwritten() == 0 and labels.check_untouched() and labels.unwritten() == 0
    assert ws.guard_intact() and gtab.changed_anywhere() == 0 and gz.changed_anywhere() == 0
    assert torch.equal(images.view.view(torch.int32), a[0].view(torch.int32))
    assert torch.equal(labels.view.view(torch.int32)[..., 0], a[1])


# ------------------------------------------------------------------------------------------------- the way back
ZOOMED = (13, 11)                    # int32((12, 10) * 1.125)


def _corners(depth):
    return [(z, y, x) for z in (0, depth - 1) for y in (0, ref.H - 1) for x in (0, ref.W - 1)]


def _case_rows(store, ci, crop, shape=SHAPE):
    """test_gpu_eval3d.py's rows -- the eight volume corners, eight overlapping interior rows with all eight flips, a few
    shifted ones -- with the issue's crop depths walking through them."""
    depth = ref.DEPTHS[ci]
    mid = (depth // 2, 19, 23)
    centres = _corners(depth) + [mid] * 8 + [(mid[0] - 1, 22, 25), (mid[0] + 1, 12, 30), (depth - 1, 39, 0)]
    tab = np.stack([ref.table_row(store.offset[ci], depth, c, crop, FLIPS[j % 8]) for j, c in enumerate(centres)])
    cds = _depths(shape, ci)
    return tab, np.array([cds[(j + j // 8) % len(cds)] for j in range(len(tab))], dtype=np.int32)


def _tables(shape, seed):
    """Positive window weights per axis with a maximum of 1, not symmetric: a wrong tap or flip shows."""
    rng = np.random.default_rng(seed)
    out = []
    for n in shape:
        g = rng.uniform(0.2, 1.0, n).astype(np.float32)
        g[rng.integers(0, n)] = 1.0
        out.append(g)
    return tuple(out)


def _accumulate(store, ci, tab, zc, probs, tables=None, zspace=True, shape=SHAPE, zmax=ZMAX):
    from boxsegliver_amd import ops
    depth = ref.DEPTHS[ci]
    c = probs.shape[-1]
    acc = torch.zeros((depth,) + HW + (c,), dtype=torch.float32, device="cuda")
    weight = torch.zeros((depth,) + HW, dtype=torch.int32 if tables is None else torch.float32, device="cuda")
    box = zref.union_box(tab, [zref.clamp_cd(v, zmax) for v in zc], depth, HW)
    kw = dict(zcrop=torch.from_numpy(np.asarray(zc, dtype=np.int32)).cuda(), zcrop_max=zmax) if zspace else {}
    dprobs = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    if tables is None:
        ops.eval3d_accumulate(dprobs, torch.from_numpy(tab).cuda(), shape, store.offset[ci], depth, box, acc, weight, store.dev_im,
                              host_tab=tab, **kw)
    else:
        dev = tuple(torch.from_numpy(g).cuda() for g in tables)
        ops.eval3d_accumulate_w(dprobs, torch.from_numpy(tab).cuda(), shape, store.offset[ci], depth, box, dev, acc, weight,
                                store.dev_im, host_tab=tab, **kw)
    return acc, weight


@pytest.mark.parametrize("weighted", [False, True])
def test_accumulate_z_matches_the_restatement(store, weighted):
    """Both entries, 13 x 11 crops, all flips, every crop depth, C = 3, on the normal and the shallow case.

    The tolerance is test_gpu_eval3d.py::test_zoomed_windows_match_the_restatement's, |acc - ref| <= 2^-24 cnt (16 max|probs| +
    |ref|), widened by one more lerp: that bound carries the three nested fp32 lerps of a contribution as 16 u M (u = 2^-24,
    M = max|probs|), the constant of the patch's image bound; the hit here nests a fourth lerp, along z, whose fraction
    fz = in_z - i0 is itself a rounded product -- the step the image bound of unetk_lits_patch3d_z takes from 16 to 24.  So
      unweighted: |acc - ref| <= 2^-24 hits (24 M + |ref|), cnt exact;
      weighted:   eval3d_weighted_ref.bound, 2^-24 hits (25 wmax M + |ref|), with 25 -> 25 + 8 + 3 = 36: the 8 of the fourth
                  lerp and 3 u wmax for the weight's own third lerp (a subtraction, a product, a sum, as wy and wx there);
                  wsum within 2^-24 hits ((8 + 3) wmax + |ref|).
    (lits3d_zspace_ref.bound / bound_wsum.)"""
    worst = 0.0
    for ci in (NORMAL, SHALLOW):
        depth = ref.DEPTHS[ci]
        tab, zc = _case_rows(store, ci, ZOOMED)
        probs = np.random.default_rng(31 + ci).random((len(tab),) + SHAPE + (3,), dtype=np.float32)
        tables = _tables(SHAPE, 37 + ci) if weighted else None
        acc, weight = _accumulate(store, ci, tab, zc, probs, tables)
        s = zref.accumulate(tab, zc, probs, SHAPE, depth, HW, tables)
        assert s.hits.max() >= 8
        hit = s.hits > 0
        if weighted:
            werr = np.abs(weight.cpu().numpy().astype(np.float64) - s.wsum)
            assert np.all(werr <= zref.bound_wsum(s)) and np.all((weight.cpu().numpy() > 0) == hit)
        else:
            np.testing.assert_array_equal(weight.cpu().numpy(), s.hits)
        err = np.abs(acc.cpu().numpy().astype(np.float64) - s.acc)
        bound = zref.bound(s, np.abs(probs).max(), weighted)
        frac = float((err[hit] / bound[hit]).max())
        print("eval3d_accumulate_{} case {}: max error / bound = {:.3f}".format("wz" if weighted else "z", ci, frac))
        worst = max(worst, frac)
        assert np.all(err <= bound), (ci, frac)
        assert np.all(err[~hit] == 0)
    assert worst > 0


@pytest.mark.parametrize("shape", [SHAPE, FLAT])
def test_accumulate_z_with_the_output_depth_equals_the_plain_entries_bit_for_bit(store, shape):
    """Every zcrop == D: acc and cnt of unetk_eval3d_accumulate, acc and wsum of unetk_eval3d_accumulate_w -- with random
    tables and with all-ones tables, which in turn give the unweighted acc."""
    for ci in (NORMAL, SHALLOW):
        crop = tuple(int(v) for v in (np.array(shape[1:]) * 1.125))
        tab, _ = _case_rows(store, ci, crop, shape)
        zc = np.full(len(tab), shape[0], np.int32)
        probs = np.random.default_rng(41 + ci).random((len(tab),) + shape + (3,), dtype=np.float32)
        plain = _accumulate(store, ci, tab, zc, probs, zspace=False, shape=shape)
        got = _accumulate(store, ci, tab, zc, probs, shape=shape)
        assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32)) and torch.equal(got[1], plain[1])
        assert int(plain[1].max()) >= 8
        ones = tuple(np.ones(n, np.float32) for n in shape)
        for tables in (_tables(shape, 43 + ci), ones):
            want = _accumulate(store, ci, tab, zc, probs, tables, zspace=False, shape=shape)
            gotw = _accumulate(store, ci, tab, zc, probs, tables, shape=shape)
            assert torch.equal(gotw[0].view(torch.int32), want[0].view(torch.int32))
            assert torch.equal(gotw[1].view(torch.int32), want[1].view(torch.int32))
        assert torch.equal(gotw[0].view(torch.int32), plain[0].view(torch.int32))     # all-ones: the unweighted sums
        assert torch.equal(gotw[1], plain[1].float())


def test_constant_windows_come_back_exactly(store):
    """Windows of one probability p, exact in float32: every lerp of equal values is exact, so acc == hits * p; with weights and
    p a power of two the products w p round as w does, so acc == p * wsum bit for bit and acc / wsum == p."""
    for ci in (NORMAL, SHALLOW):
        tab, zc = _case_rows(store, ci, ZOOMED)
        for p in (0.5, 0.375):
            probs = np.full((len(tab),) + SHAPE + (2,), p, np.float32)
            acc, cnt = _accumulate(store, ci, tab, zc, probs)
            assert int(cnt.max()) >= 8
            assert torch.equal(acc, cnt.float()[..., None].expand_as(acc) * p)
        probs = np.full((len(tab),) + SHAPE + (2,), 0.5, np.float32)
        acc, wsum = _accumulate(store, ci, tab, zc, probs, _tables(SHAPE, 47))
        hit = wsum > 0
        assert torch.equal(hit, cnt > 0)
        assert torch.equal(acc, wsum[..., None].expand_as(acc) * 0.5)
        assert bool(((acc[hit] / wsum[hit][:, None]) == 0.5).all())


def test_guard_bands_and_arguments_of_the_way_back(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    ci, depth = SHALLOW, ref.DEPTHS[SHALLOW]
    tab, zc = _case_rows(store, ci, ZOOMED)
    n = len(tab)
    probs = np.random.default_rng(53).random((n,) + SHAPE + (3,), dtype=np.float32)
    tables = _tables(SHAPE, 59)
    want, wantw = _accumulate(store, ci, tab, zc, probs), _accumulate(store, ci, tab, zc, probs, tables)
    box = (ctypes.c_int32 * 6)(*zref.union_box(tab, zc, depth, HW))
    desc = ops.lits3d_desc(store.dev_im, n, SHAPE, False)
    gprobs = guardbuf.guarded_input(torch.from_numpy(probs).cuda())
    gtab = guardbuf.guarded_input(torch.from_numpy(tab.view(np.float32)).cuda())
    gzc = guardbuf.guarded_input(torch.from_numpy(zc.view(np.float32)[:, None]).cuda())
    dev = [torch.from_numpy(g).cuda() for g in tables]
    for weighted in (False, True):
        acc, wgt = guardbuf.guarded((depth,) + HW + (3,)), guardbuf.guarded((depth,) + HW + (1,))
        for g in (acc, wgt):
            g.view.view(torch.int32).zero_()
            g.snap = g.flat.clone()

        def call(z=gzc.ptr(), zmax=ZMAX):
            head = (ctypes.byref(desc), ctypes.c_void_p(gtab.ptr()), ctypes.c_void_p(z), zmax, ctypes.c_void_p(gprobs.ptr()), 3,
                    store.offset[ci], depth, box)
            if weighted:
                return lib.unetk_eval3d_accumulate_wz(*head, _abi.ptr(dev[0]), _abi.ptr(dev[1]), _abi.ptr(dev[2]),
                                                      ctypes.c_void_p(acc.ptr()), ctypes.c_void_p(wgt.ptr()), _abi.stream_ptr())
            return lib.unetk_eval3d_accumulate_z(*head, ctypes.c_void_p(acc.ptr()), ctypes.c_void_p(wgt.ptr()), _abi.stream_ptr())
        assert call(z=None) == -1 and call(z=gzc.ptr() + 1) == -1 and call(zmax=0) == -1
        assert call(zmax=-(-(1 << 31) // (ref.H * ref.W))) == -2
        torch.cuda.synchronize()
        assert acc.changed_anywhere() == 0 and wgt.changed_anywhere() == 0
        assert call() == 0
        torch.cuda.synchronize()
        assert acc.check_untouched() and wgt.check_untouched()
        assert gprobs.changed_anywhere() == 0 and gtab.changed_anywhere() == 0 and gzc.changed_anywhere() == 0
        ref_acc, ref_w = wantw if weighted else want
        assert torch.equal(acc.view.view(torch.int32), ref_acc.view(torch.int32))
        assert torch.equal(wgt.view.view(torch.int32)[..., 0], ref_w.view(torch.int32))


# ------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("cd", [SHAPE[0] - 1, SHAPE[0], 2 * SHAPE[0] + 1])
def test_round_trip_through_both_kernels(store, cd):
    """Case 0 (12 slices) tiled along z by the host's own window_starts(depth, cd, 0.5) -- 12 is no multiple of the step for
    cd = 9 (step 4: starts 0, 3) -- and in the plane by windows of the patch's own size (zoom 1); the windows cut by
    unetk_lits_patch3d_z, one-hot "probabilities" of their labels taken back by unetk_eval3d_accumulate_z and
    unetk_eval3d_finish: no voxel is left uncovered, and with cd == D the argmax is the stored label everywhere."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits3d
    ci, depth = NORMAL, ref.DEPTHS[NORMAL]
    im, lb = store.cases[ci]
    h, w = SHAPE[1:]
    starts = lits3d.window_starts(depth, cd, 0.5)
    assert starts[0] == 0 and starts[-1] + cd == depth and (cd != 9 or starts == [0, 3])
    rows = [ref.table_row(store.offset[ci], depth, (z + cd // 2, y + h // 2, x + w // 2), (h, w))
            for z in starts for y in lits3d.window_starts(ref.H, h, 0.5) for x in lits3d.window_starts(ref.W, w, 0.5)]
    tab = np.stack(rows)
    zc = np.full(len(tab), cd, np.int32)
    assert lits3d.table_box(tab, SHAPE, depth, HW, cd=cd) == (0, depth, 0, ref.H, 0, ref.W) == zref.union_box(tab, zc, depth, HW)
    dtab, dz = torch.from_numpy(tab).cuda(), torch.from_numpy(zc).cuda()
    _, labels = ops.lits_patch3d(store.dev_im, store.dev_lb, dtab, SHAPE, False, 2, zcrop=dz, zcrop_max=cd)
    probs = torch.zeros(labels.shape + (3,), dtype=torch.float32, device="cuda")
    probs.scatter_(-1, labels.long().unsqueeze(-1), 1.0)
    acc = torch.zeros((depth,) + HW + (3,), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((depth,) + HW, dtype=torch.int32, device="cuda")
    whole = (0, depth, 0, ref.H, 0, ref.W)
    ops.eval3d_accumulate(probs, dtab, SHAPE, store.offset[ci], depth, whole, acc, cnt, store.dev_im, host_tab=tab, zcrop=dz,
                          zcrop_max=cd)
    uncovered = torch.zeros(1, dtype=torch.int32, device="cuda")
    pred = ops.eval3d_finish(acc, cnt, whole, uncovered).cpu().numpy()
    assert int(uncovered.item()) == 0 and int(cnt.min()) >= 1
    agree = float((pred == lb).mean())
    print("round trip cd = {}: {} windows, argmax == label on {:.4f} of the voxels".format(cd, len(tab), agree))
    if cd == SHAPE[0]:
        np.testing.assert_array_equal(pred, lb)
