"""GPU: volume evaluation on the device (csrc/evalvol.hip, ops.largest_component3d / mask_counts / surface_distances,
loss_metrics.metric_3d_device, EvaluateVolume(metrics_on="device")) against the host functions it restates
(array_kits.get_largest_component, ConfusionMatrix, Surface, scipy's distance transform, metric_3d)."""
import ctypes
import math
import os
import time

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from guardbuf import GuardedWorkspace

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLINGS = [(1.0, 1.0, 1.0), (2.5, 0.7, 0.7), (5.0, 0.78125, 0.78125)]
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3


def _lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


def _st():
    from boxsegliver_amd._abi import stream_ptr
    return stream_ptr()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _blob(rng, shape, density, sigma=1.0):
    """Thresholded smoothed noise with the given fraction of object voxels."""
    x = ndi.gaussian_filter(rng.random(shape), sigma)
    return x > np.quantile(x, 1.0 - density)


def _host_lc(m):
    from boxsegliver_amd.utils import array_kits
    return array_kits.get_largest_component(m, rank=3).astype(np.uint8)


def _dev_lc(m):
    from boxsegliver_amd import ops
    return ops.largest_component3d(_dev(m.astype(np.uint8))).cpu().numpy()


# ------------------------------------------------------------------------------------------------ largest component
def test_largest_component_random_volumes():
    rng = np.random.default_rng(11)
    shapes = [(9, 17, 23), (16, 31, 40), (5, 64, 64), (24, 20, 33)]
    for t in range(32):
        shape = shapes[t % len(shapes)]
        m = _blob(rng, shape, rng.uniform(0.05, 0.6), sigma=rng.uniform(0.6, 1.6))
        np.testing.assert_array_equal(_dev_lc(m), _host_lc(m), err_msg=str(t))


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 40, 56), (30, 1, 45), (7, 13, 17), (64, 97, 131)])
def test_largest_component_shapes_empty_full_single(shape):
    rng = np.random.default_rng(sum(shape))
    cases = [np.zeros(shape, bool), np.ones(shape, bool)]
    single = np.zeros(shape, bool)
    single[tuple(s // 2 for s in shape)] = True
    cases.append(single)
    if np.prod(shape) > 1:
        cases += [_blob(rng, shape, d) for d in (0.1, 0.3, 0.55)]
    for i, m in enumerate(cases):
        got = _dev_lc(m)
        np.testing.assert_array_equal(got, _host_lc(m), err_msg="{} case {}".format(shape, i))
    assert not _dev_lc(cases[0]).any() and _dev_lc(cases[1]).all()


def test_largest_component_diagonal_contacts_do_not_merge():
    m = np.zeros((6, 7, 8), bool)
    m[1, 1, 1:4] = True          # a 3-voxel run
    m[2, 2, 4] = True            # touches its end across an edge+corner only
    m[1, 2, 4] = True            # ... and this one across an edge: 2 voxels together, still apart from the run
    m[3, 4, 5:7] = True
    m[4, 5, 7] = True            # corner-only contact
    got = _dev_lc(m)
    np.testing.assert_array_equal(got, _host_lc(m))
    assert got.sum() == 3 and got[1, 1, 1:4].all()
    # a 2x2x2 checkerboard: four voxels with only edge contacts, four one-voxel components; the tie goes to the last one in
    # raster order (a handful of components: np.argsort, behind the host's tie rule, is stable only for short arrays)
    z, y, x = np.indices((2, 2, 2))
    cb = (z + y + x) % 2 == 0
    got = _dev_lc(cb)
    np.testing.assert_array_equal(got, _host_lc(cb))
    assert got.sum() == 1 and got.flat[np.flatnonzero(cb)[-1]] == 1


def _serpentine(D, H, W):
    """One 6-connected path through every other row of every plane, planes joined at alternating ends."""
    m = np.zeros((D, H, W), bool)
    for z in range(D):
        rows = list(range(0, H, 2))
        if z % 2:
            rows = rows[::-1]
        for j, y in enumerate(rows):
            m[z, y, :] = True
            if j + 1 < len(rows):
                x = W - 1 if (j % 2 == 0) != bool(z % 2) else 0
                m[z, min(y, rows[j + 1]):max(y, rows[j + 1]) + 1, x] = True
    return m


def test_largest_component_serpentine_and_spiral_across_blocks():
    m = _serpentine(12, 41, 67)
    lab, n = ndi.label(m, ndi.generate_binary_structure(3, 1))
    assert n == 1
    specks = np.random.default_rng(3).random(m.shape) < 0.02
    m2 = m | (specks & ~ndi.binary_dilation(m, ndi.generate_binary_structure(3, 1)))
    for vol in (m, m2):
        got = _dev_lc(vol)
        np.testing.assert_array_equal(got, _host_lc(vol))
    assert np.array_equal(_dev_lc(m2), m.astype(np.uint8))
    # a square spiral in one plane, extruded through depth with gaps: one long chain per plane, joined at one corner
    sp = np.zeros((4, 63, 63), bool)
    y, x, dy, dx, step = 31, 31, 0, 1, 1
    sp[:, y, x] = True
    while 0 < y < 62 and 0 < x < 62:
        for _ in range(2):
            for _ in range(step):
                ny, nx = y + dy, x + dx
                if not (0 <= ny < 63 and 0 <= nx < 63):
                    break
                y, x = ny, nx
                sp[0, y, x] = sp[2, y, x] = True
            dy, dx = dx, -dy
        step += 2
    sp[1, 31, 31] = True
    got = _dev_lc(sp)
    np.testing.assert_array_equal(got, _host_lc(sp))


def test_largest_component_ties_take_the_larger_root():
    m = np.zeros((10, 12, 14), bool)
    m[1:3, 1:3, 1:3] = True
    m[6:8, 7:9, 9:11] = True             # same size, later in raster order
    got = _dev_lc(m)
    np.testing.assert_array_equal(got, _host_lc(m))
    assert got[6:8, 7:9, 9:11].all() and not got[1:3, 1:3, 1:3].any()
    m[4, 1, 10:12] = True
    m[4, 1, 12] = True                   # three of size 8 / 8 / 3 ... and a third 8-cube first in raster order
    m[0, 8:10, 0:2] = True
    m[1, 8:10, 0:2] = True
    np.testing.assert_array_equal(_dev_lc(m), _host_lc(m))


def test_largest_component_many_equal_components_follow_the_host_argsort():
    """More than 16 components sharing the largest size: the host's pick is whatever np.argsort's (unstable) sort puts
    last; the device reproduces it from its component table."""
    rng = np.random.default_rng(6)
    for t in range(4):
        m = np.zeros((12, 40, 44), bool)
        for k in range(int(rng.integers(20, 60))):                     # equal 2x2x2 cubes on a lattice, some smaller bits
            z, y, x = 3 * (k % 4), 4 * ((k // 4) % 10), 4 * (k // 40) + 4 * int(rng.integers(0, 10))
            m[z:z + 2, y:y + 2, x:x + 2] = True
        m[rng.random(m.shape) < 0.002] = True
        np.testing.assert_array_equal(_dev_lc(m), _host_lc(m), err_msg=str(t))
    iso = np.zeros((9, 9, 9), bool)
    iso[::2, ::2, ::2] = True                                          # 125 single voxels
    np.testing.assert_array_equal(_dev_lc(iso), _host_lc(iso))


# ------------------------------------------------------------------------------------------------ counts / surface
def test_mask_counts_equal_numpy_and_confusion_matrix():
    from boxsegliver_amd import loss_metrics, ops
    rng = np.random.default_rng(5)
    for t in range(12):
        shape = tuple(int(s) for s in rng.integers(1, 40, 3))
        a = (rng.random(shape) < rng.uniform(0, 0.7)).astype(np.uint8) * rng.choice([1, 2, 255])
        b = (rng.random(shape) < rng.uniform(0, 0.7)).astype(np.uint8)
        c = ops.mask_counts(_dev(a), _dev(b))
        ab, bb = a != 0, b != 0
        assert (c["na"], c["nb"], c["inter"], c["union"]) == (np.count_nonzero(ab), np.count_nonzero(bb),
                                                               np.count_nonzero(ab & bb), np.count_nonzero(ab | bb))
        conf = loss_metrics.ConfusionMatrix(a.astype(int), b.astype(int))
        conf.compute()
        assert (c["tp"], c["fp"], c["fn"]) == (conf.tp, conf.fp, conf.fn)
        assert all(type(v) is int for v in c.values())


def _surface(m, box=None, accumulate=False):
    d, h, w = m.shape
    edge = torch.empty((d, h, w), dtype=torch.uint8, device="cuda")
    box = torch.empty(6, dtype=torch.int32, device="cuda") if box is None else box
    assert _lib().unetk_surface3d(_dev(m.astype(np.uint8)).data_ptr(), d, h, w, edge.data_ptr(), box.data_ptr(),
                                  int(accumulate), _st()) == 0
    return edge, box


def _bbox(m):
    idx = np.argwhere(m)
    return list(idx.min(0)) + list(idx.max(0) + 1)


def test_surface_equals_compute_contour_and_box():
    from boxsegliver_amd.utils.surface import Surface
    rng = np.random.default_rng(8)
    for t in range(14):
        shape = tuple(int(s) for s in rng.integers(1, 35, 3))
        m = _blob(rng, shape, rng.uniform(0.05, 0.9)) if min(shape) > 1 else rng.random(shape) < 0.5
        edge, box = _surface(m)
        ref = Surface.compute_contour(m)
        np.testing.assert_array_equal(edge.cpu().numpy(), ref.astype(np.uint8), err_msg=str(t))
        if ref.any():
            assert box.cpu().tolist() == _bbox(ref)
        else:
            assert box.cpu().tolist()[3:] == [0, 0, 0]
    # the union box of two surfaces
    a, b = np.zeros((9, 10, 11), bool), np.zeros((9, 10, 11), bool)
    a[1:3, 2:4, 3:5] = True
    b[5:8, 6:9, 7:10] = True
    _, box = _surface(a)
    _, box = _surface(b, box, accumulate=True)
    assert box.cpu().tolist() == [1, 2, 3, 8, 9, 10]


# ------------------------------------------------------------------------------------------------ distance transform
def _edt(feature, box_list, sampling):
    d, h, w = feature.shape
    lib = _lib()
    box = torch.tensor(box_list, dtype=torch.int32, device="cuda")
    dist2 = torch.full((d, h, w), -1.0, dtype=torch.float64, device="cuda")
    nbytes = lib.unetk_edt3d_sq_ws_bytes(d, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    f = _dev(feature.astype(np.uint8))
    assert lib.unetk_edt3d_sq(f.data_ptr(), d, h, w, box.data_ptr(), *[ctypes.c_double(s) for s in sampling],
                              dist2.data_ptr(), ws.data_ptr(), nbytes, _st()) == 0
    return dist2.cpu().numpy()


def _rel_close(got, ref, tol=1e-12):
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    return bool(np.all(np.where(ref == 0, got == 0, err <= tol)))


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_edt_equals_scipy_inside_the_box(sampling):
    from boxsegliver_amd.utils.surface import Surface
    rng = np.random.default_rng(int(sampling[0] * 10))
    for t in range(8):
        shape = tuple(int(s) for s in rng.integers(2, 48, 3))
        m = _blob(rng, shape, rng.uniform(0.05, 0.5))
        edge = Surface.compute_contour(m) if t % 2 == 0 else rng.random(shape) < 0.002
        if not edge.any():
            edge.flat[rng.integers(edge.size)] = True
        box = _bbox(edge)
        if t % 3 == 0:        # a larger box than the features' own is exact too
            box = [max(0, box[0] - 1), 0, max(0, box[2] - 2), shape[0], min(shape[1], box[4] + 3), shape[2]]
        got = _edt(edge, box, sampling)
        ref = ndi.distance_transform_edt(~edge, sampling=sampling) ** 2
        sl = tuple(slice(box[k], box[k + 3]) for k in range(3))
        assert _rel_close(got[sl], ref[sl]), (t, np.abs(got[sl] - ref[sl]).max())
        outside = np.ones(shape, bool)
        outside[sl] = False
        assert np.all(got[outside] == -1.0)                 # nothing written outside the box


# ------------------------------------------------------------------------------------------------ metric_3d_device
def _same_metrics(dev, host, exact=("Dice", "VOE", "RVD"), tol=1e-12):
    assert list(dev) == list(host), (list(dev), list(host))
    for k in host:
        assert type(dev[k]) is type(host[k]), (k, type(dev[k]), type(host[k]))
        if k in exact or host[k] == 0 or (isinstance(host[k], float) and math.isnan(host[k])):
            assert dev[k] == host[k] or (math.isnan(dev[k]) and math.isnan(host[k])), (k, dev[k], host[k])
        else:
            assert abs(dev[k] - host[k]) <= tol * abs(host[k]), (k, dev[k], host[k])


def test_metric_3d_device_equals_metric_3d_on_random_pairs():
    from boxsegliver_amd.loss_metrics import metric_3d, metric_3d_device
    rng = np.random.default_rng(21)
    for t in range(24):
        shape = tuple(int(s) for s in rng.integers(4, 40, 3))
        a = _blob(rng, shape, rng.uniform(0.05, 0.5))
        b = ndi.binary_dilation(a, iterations=int(rng.integers(0, 2))) ^ (rng.random(shape) < 0.03)
        s = SAMPLINGS[t % 3]
        _same_metrics(metric_3d_device(_dev(a), _dev(b), sampling=s), metric_3d(a, b, sampling=s))
        _same_metrics(metric_3d_device(_dev(a), _dev(b), required=["Dice", "MSD"], sampling=s),
                      metric_3d(a, b, required=["Dice", "MSD"], sampling=s))
    # numpy inputs are accepted (uploaded once)
    _same_metrics(metric_3d_device(a, b, required="ASSD"), metric_3d(a, b, required="ASSD"))


def test_metric_3d_device_edge_cases():
    from boxsegliver_amd.loss_metrics import metric_3d, metric_3d_device
    shape = (6, 7, 8)
    empty, full = np.zeros(shape, bool), np.ones(shape, bool)
    one = np.zeros(shape, bool)
    one[3, 3, 3] = True
    other = np.zeros(shape, bool)
    other[0, 6, 7] = True
    no_rvd = ["Dice", "VOE", "ASSD", "RMSD", "MSD"]
    for a, b in ((empty, empty), (empty, one), (full, full), (one, one), (one, other), (full, one), (one, full)):
        req = None if b.any() else no_rvd
        _same_metrics(metric_3d_device(_dev(a), _dev(b), required=req), metric_3d(a, b, required=req))
    for a, b in ((one, empty), (empty, empty)):
        with pytest.raises(RuntimeError):
            metric_3d(a, b, required=["RVD"])
        with pytest.raises(RuntimeError):
            metric_3d_device(_dev(a), _dev(b), required=["RVD"])
    with pytest.raises(ValueError):
        metric_3d_device(_dev(one), _dev(one), required=["Dice", "HD95"])
    r = metric_3d_device(_dev(empty), _dev(empty), required=no_rvd)
    assert r["Dice"] == 0.0 and math.isnan(r["VOE"]) and r["ASSD"] == 0 and r["MSD"] == 0 and "RMSD" not in r
    # 4-D inputs are squeezed like the host's
    _same_metrics(metric_3d_device(_dev(one[None]), _dev(full[..., None])), metric_3d(one[None], full[..., None]))


def test_metric_3d_device_reproduces_the_reference_surface_fixtures():
    from boxsegliver_amd.loss_metrics import metric_3d_device
    d = np.load(os.path.join(HERE, "golden", "ref_surface.npz"))
    for i in range(len(d["assd"])):
        sz, sy, sx = d["shapes"][i]
        a = np.unpackbits(d["masks"][i]).reshape(16, 30, 24)[:sz, :sy, :sx].astype(bool)
        b = np.unpackbits(d["refs"][i]).reshape(16, 30, 24)[:sz, :sy, :sx].astype(bool)
        m = metric_3d_device(_dev(a), _dev(b), required=["ASSD", "RMSD", "MSD"], sampling=list(d["spacings"][i]))
        assert m["ASSD"] == pytest.approx(d["assd"][i], rel=1e-10, abs=1e-12), i
        assert m["RMSD"] == pytest.approx(d["rmsd"][i], rel=1e-10, abs=1e-12), i
        assert m["MSD"] == pytest.approx(d["msd"][i], rel=1e-10, abs=1e-12), i


def test_device_results_are_bit_identical_across_runs():
    from boxsegliver_amd import ops
    from boxsegliver_amd.loss_metrics import metric_3d_device
    rng = np.random.default_rng(2)
    a = _dev(_blob(rng, (40, 90, 70), 0.3))
    b = _dev(_blob(rng, (40, 90, 70), 0.35))
    r1 = (ops.largest_component3d(a).cpu(), ops.surface_distances(a, b, (2.5, 0.7, 0.7)),
          metric_3d_device(a, b, sampling=(2.5, 0.7, 0.7)))
    r2 = (ops.largest_component3d(a).cpu(), ops.surface_distances(a, b, (2.5, 0.7, 0.7)),
          metric_3d_device(a, b, sampling=(2.5, 0.7, 0.7)))
    assert torch.equal(r1[0], r2[0])
    assert r1[1] == r2[1]                                            # float == : bit-identical sums
    assert r1[2] == r2[2]


# ------------------------------------------------------------------------------------------------ guard bands / refusals
class _GBytes(object):
    """A device byte buffer through tests/guardbuf.GuardedWorkspace: exactly `data.nbytes` (or nbytes) at 16 (mod 256),
    a sentinel guard behind it; inputs hold their data, outputs start with a pattern no kernel writes."""

    def __init__(self, data=None, nbytes=None, fill=0xA5):
        self.ws = GuardedWorkspace(data.nbytes if data is not None else nbytes)
        if data is not None:
            self.ws.buf[self.ws.off:self.ws.off + data.nbytes].copy_(_dev(np.frombuffer(data.tobytes(), np.uint8)))
        else:
            self.ws.fill(fill)
        self.start = self.payload().clone()

    def payload(self):
        return self.ws.buf[self.ws.off:self.ws.off + self.ws.nbytes]

    def ptr(self):
        return self.ws.ptr()

    def as_np(self, dtype, shape):
        return self.payload().cpu().numpy().view(dtype).reshape(shape)


def _guard_rows():
    rng = np.random.default_rng(17)
    for shape in ((7, 13, 17), (5, 33, 64), (1, 9, 250)):
        a = _blob(rng, shape, 0.3) if min(shape) > 1 else rng.random(shape) < 0.4
        b = _blob(rng, shape, 0.25) if min(shape) > 1 else rng.random(shape) < 0.4
        yield shape, a.astype(np.uint8), b.astype(np.uint8)


def test_guard_bands_of_every_new_output_and_workspace():
    from boxsegliver_amd.utils.surface import Surface
    lib, st = _lib(), _st()
    for shape, a, b in _guard_rows():
        d, h, w = shape
        ga, gb = _GBytes(a), _GBytes(b)
        results = []
        for fill in (0x00, 0xFF, 0x5A):
            out = {}
            # largest component
            nb = lib.unetk_largest_component_ws_bytes(d, h, w)
            ws, o, info = GuardedWorkspace(nb), _GBytes(nbytes=a.size), _GBytes(nbytes=16)
            ws.fill(fill)
            assert lib.unetk_largest_component(ga.ptr(), d, h, w, o.ptr(), info.ptr(), ws.ptr(), nb, st) == 0
            torch.cuda.synchronize()
            assert ws.guard_intact() and o.ws.guard_intact() and info.ws.guard_intact()
            out["lc"] = o.as_np(np.uint8, shape).copy()
            np.testing.assert_array_equal(out["lc"], _host_lc(a.astype(bool)))
            lab, ncomp = ndi.label(a, ndi.generate_binary_structure(3, 1))
            areas = np.bincount(lab.flat)[1:]
            root = int(np.flatnonzero(out["lc"])[0])
            assert info.as_np(np.int32, (4,)).tolist() == [root, areas.max(), (areas == areas.max()).sum(), ncomp]
            out["info"] = info.as_np(np.int32, (4,)).copy()
            o2 = _GBytes(nbytes=a.size)                    # the table left in the workspace: the component rooted at voxel 0
            assert lib.unetk_component_mask(ws.ptr(), d, h, w, 0, o2.ptr(), st) == 0
            torch.cuda.synchronize()
            assert o2.ws.guard_intact() and ws.guard_intact()
            np.testing.assert_array_equal(o2.as_np(np.uint8, shape), (lab == 1) if a.flat[0] else np.zeros(shape, np.uint8))
            # counts
            nb = lib.unetk_mask_counts_ws_bytes(d, h, w)
            ws, o = GuardedWorkspace(nb), _GBytes(nbytes=32)
            ws.fill(fill)
            assert lib.unetk_mask_counts(ga.ptr(), gb.ptr(), d, h, w, o.ptr(), ws.ptr(), nb, st) == 0
            torch.cuda.synchronize()
            assert ws.guard_intact() and o.ws.guard_intact()
            out["counts"] = o.as_np(np.int64, (4,)).copy()
            ab, bb = a != 0, b != 0
            assert out["counts"].tolist() == [ab.sum(), bb.sum(), (ab & bb).sum(), (ab | bb).sum()]
            # surfaces + union box
            ea, eb, box = _GBytes(nbytes=a.size), _GBytes(nbytes=a.size), _GBytes(nbytes=24)
            assert lib.unetk_surface3d(ga.ptr(), d, h, w, ea.ptr(), box.ptr(), 0, st) == 0
            assert lib.unetk_surface3d(gb.ptr(), d, h, w, eb.ptr(), box.ptr(), 1, st) == 0
            torch.cuda.synchronize()
            assert ea.ws.guard_intact() and eb.ws.guard_intact() and box.ws.guard_intact()
            sa, sb = Surface.compute_contour(ab), Surface.compute_contour(bb)
            np.testing.assert_array_equal(ea.as_np(np.uint8, shape), sa.astype(np.uint8))
            np.testing.assert_array_equal(eb.as_np(np.uint8, shape), sb.astype(np.uint8))
            bx = box.as_np(np.int32, (6,)).tolist()
            assert bx == _bbox(sa | sb)
            # distance transform over the box, then the sums
            nb = lib.unetk_edt3d_sq_ws_bytes(d, h, w)
            ws, dist = GuardedWorkspace(nb), _GBytes(nbytes=a.size * 8)
            ws.fill(fill)
            assert lib.unetk_edt3d_sq(eb.ptr(), d, h, w, box.ptr(), ctypes.c_double(2.5), ctypes.c_double(0.7),
                                      ctypes.c_double(0.7), dist.ptr(), ws.ptr(), nb, st) == 0
            torch.cuda.synchronize()
            assert ws.guard_intact() and dist.ws.guard_intact()
            sl = tuple(slice(bx[k], bx[k + 3]) for k in range(3))
            got = dist.as_np(np.float64, shape)
            ref = ndi.distance_transform_edt(~sb, sampling=(2.5, 0.7, 0.7)) ** 2
            assert _rel_close(got[sl], ref[sl])
            out["edt"] = got[sl].copy()
            nb = lib.unetk_surface_dist_ws_bytes(d, h, w)
            ws, o = GuardedWorkspace(nb), _GBytes(nbytes=32)
            ws.fill(fill)
            assert lib.unetk_surface_dist(ea.ptr(), dist.ptr(), d, h, w, o.ptr(), ws.ptr(), nb, st) == 0
            torch.cuda.synchronize()
            assert ws.guard_intact() and o.ws.guard_intact()
            sums = o.as_np(np.float64, (4,)).copy()
            dd = np.sqrt(ref[sa])
            assert sums[:3] == pytest.approx([dd.sum(), (dd * dd).sum(), dd.max()], rel=1e-12)
            assert sums.view(np.int64)[3] == sa.sum()
            out["sums"] = sums
            # inputs untouched
            assert torch.equal(ga.payload(), ga.start) and torch.equal(gb.payload(), gb.start)
            assert ga.ws.guard_intact() and gb.ws.guard_intact()
            results.append(out)
        for r in results[1:]:                                             # three workspace fills, bit-equal results
            for k in r:
                assert np.array_equal(r[k].view(np.uint8), results[0][k].view(np.uint8)), k


def test_refusals_null_misaligned_short_workspace_and_too_many_voxels():
    lib, st = _lib(), _st()
    d, h, w = 7, 13, 17
    m = torch.ones((d, h, w), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(m)
    dist = torch.empty((d, h, w), dtype=torch.float64, device="cuda")
    box = torch.zeros(6, dtype=torch.int32, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    big = 1 << 20
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    P = lambda t: t.data_ptr()
    c = ctypes.c_double(1.0)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls = {     # name -> (workspace bytes, call(input, output, ws, ws_bytes), a valid output)
        "lc": (lib.unetk_largest_component_ws_bytes(d, h, w),
               lambda mk, o, wsp, n: lib.unetk_largest_component(mk, d, h, w, o, P(info), wsp, n, st), P(out)),
        "counts": (lib.unetk_mask_counts_ws_bytes(d, h, w),
                   lambda mk, o, wsp, n: lib.unetk_mask_counts(mk, mk, d, h, w, o, wsp, n, st), P(res)),
        "edt": (lib.unetk_edt3d_sq_ws_bytes(d, h, w),
                lambda mk, o, wsp, n: lib.unetk_edt3d_sq(mk, d, h, w, P(box), c, c, c, o, wsp, n, st), P(dist)),
        "sdist": (lib.unetk_surface_dist_ws_bytes(d, h, w),
                  lambda mk, o, wsp, n: lib.unetk_surface_dist(mk, P(dist), d, h, w, o, wsp, n, st), P(res)),
    }
    for name, (nbytes, fn, o) in calls.items():
        assert 0 < nbytes < big, name
        assert fn(None, o, P(ws), nbytes) == E_BADARG, name                    # NULL input
        assert fn(P(m), None, P(ws), nbytes) == E_BADARG, name                 # NULL output
        assert fn(P(m), o, None, nbytes) == E_BADARG, name                     # NULL workspace
        assert fn(P(m), o, P(ws) + 8, nbytes) == E_BADARG, name                # misaligned workspace
        assert fn(P(m), o, P(ws), nbytes - 16) == E_WORKSPACE, name            # short workspace
        assert fn(P(m), o, P(ws), nbytes) == 0, name
    nb = lib.unetk_largest_component_ws_bytes(d, h, w)
    assert lib.unetk_largest_component(P(m), d, h, w, P(out), None, P(ws), nb, st) == E_BADARG          # NULL info
    assert lib.unetk_largest_component(P(m), d, h, w, P(out), P(info) + 2, P(ws), nb, st) == E_BADARG
    assert lib.unetk_component_mask(None, d, h, w, 0, P(out), st) == E_BADARG
    assert lib.unetk_component_mask(P(ws), d, h, w, 0, None, st) == E_BADARG
    assert lib.unetk_component_mask(P(ws) + 8, d, h, w, 0, P(out), st) == E_BADARG
    assert lib.unetk_component_mask(P(ws), d, h, w, -1, P(out), st) == E_BADARG
    assert lib.unetk_component_mask(P(ws), d, h, w, d * h * w, P(out), st) == E_BADARG
    assert lib.unetk_surface3d(None, d, h, w, P(out), P(box), 0, st) == E_BADARG
    assert lib.unetk_surface3d(P(m), d, h, w, P(out), None, 0, st) == E_BADARG
    assert lib.unetk_surface3d(P(m), d, h, w, P(out), P(box) + 2, 0, st) == E_BADARG
    assert lib.unetk_edt3d_sq(P(m), d, h, w, P(box), ctypes.c_double(0.0), c, c, P(dist), P(ws), big, st) == E_BADARG
    torch.cuda.synchronize()
    # more than 2^31 voxels: refused from the descriptor alone (nothing allocated, nothing launched)
    D, H, W = 2048, 1024, 1024
    for q in ("largest_component", "mask_counts", "edt3d_sq", "surface_dist"):
        assert getattr(lib, "unetk_{}_ws_bytes".format(q))(D, H, W) == 0
    assert lib.unetk_largest_component(None, D, H, W, None, None, None, 0, st) == E_UNSUPPORTED
    assert lib.unetk_component_mask(None, D, H, W, 0, None, st) == E_UNSUPPORTED
    assert lib.unetk_mask_counts(None, None, D, H, W, None, None, 0, st) == E_UNSUPPORTED
    assert lib.unetk_surface3d(None, D, H, W, None, None, 0, st) == E_UNSUPPORTED
    assert lib.unetk_edt3d_sq(None, D, H, W, None, c, c, c, None, None, 0, st) == E_UNSUPPORTED
    assert lib.unetk_surface_dist(None, None, D, H, W, None, None, 0, st) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the evaluator
def _lits_args(tmp_path, depth, size, **over):
    import test_gpu_unet as t
    from test_lits_eval_host import _write_dataset
    from boxsegliver_amd.NetworksV2.UNet import UNet
    _write_dataset(tmp_path, depth=depth, size=size)
    kw = dict(batch_size=4, im_height=64, im_width=64, eval_mirror=False, random_flip=3,
              metrics_eval=["Dice", "VOE", "RVD", "ASSD", "RMSD", "MSD"], use_global_dice=False, pred_type="pred",
              mode="eval", eval_num=-1, save_path=None, test_fold=2, filter_size=0, eval_skip_num=0,
              eval_in_patches=False, model="UNet")
    kw.update(over)
    args = t.make_args(**kw)
    yml = dict(t.YML, num_down_samples=3)
    return {"args": args, "model": UNet, "model_kwargs": yml, "model_args": (), "lits_root": tmp_path, "proj_root": tmp_path}


def _assert_results_match(dev, host):
    assert set(dev) == set(host)
    for k in host:
        if isinstance(host[k], float) and math.isnan(host[k]):
            assert math.isnan(dev[k]), k
        else:
            assert abs(dev[k] - host[k]) <= 1e-12 * max(1.0, abs(host[k])), (k, dev[k], host[k])


@pytest.mark.parametrize("mode", ["plain", "mirror", "patches", "global_dice"])
def test_evaluator_device_equals_host(tmp_path, mode):
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    over = {"plain": {}, "mirror": {"eval_mirror": True}, "patches": {"eval_in_patches": True, "batch_size": 5},
            "global_dice": {"use_global_dice": True}}[mode]
    params = _lits_args(tmp_path, 9, 128 if mode == "patches" else 96, **over)
    res = {}
    for on in ("host", "device"):
        e = ev.get_evaluator("Volume", estimator=None, model_dir=str(tmp_path), params=params, metrics_on=on)
        assert e.metrics_on == on
        res[on] = e.run(lits.input_fn_eval, checkpoint_path=None)      # the same model instance: the same weights
        assert e.calls == 2
    _assert_results_match(res["device"], res["host"])
    assert ("LiverDice" in res["device"]) == (mode == "global_dice")
    with pytest.raises(ValueError):
        ev.EvaluateVolume(params=params, metrics_on="gpu")


def test_evaluator_postprocess_device_equals_host():
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    from test_evaluator_host import _evaluator
    e = _evaluator()
    rng = np.random.default_rng(4)
    vol = (rng.random((12, 30, 31)) < 0.4).astype(np.uint8) + (rng.random((12, 30, 31)) < 0.2).astype(np.uint8)
    host = e._postprocess(vol.copy())
    dev = e._postprocess_device(_dev(vol))
    for cls in host:
        np.testing.assert_array_equal(dev[cls].cpu().numpy(), host[cls].astype(np.uint8), err_msg=cls)
    host = e._postprocess(vol.copy(), is_label=True)
    dev = e._postprocess_device(_dev(vol), is_label=True)
    for cls in host:
        np.testing.assert_array_equal(dev[cls].cpu().numpy(), host[cls].astype(np.uint8), err_msg=cls)
    assert isinstance(e, ev.EvaluateVolume)


@pytest.mark.parametrize("use_global_dice", [False, True])
def test_online_3d_evaluation_device_equals_host(tmp_path, use_global_dice):
    import test_gpu_unet as t
    from test_gpu_lits import _write_dataset
    from boxsegliver_amd.NetworksV2.UNet import UNet
    from boxsegliver_amd.core import estimator as est
    from boxsegliver_amd.core import models
    from boxsegliver_amd.core.solver import Solver
    from boxsegliver_amd.data import lits
    from boxsegliver_amd.evaluators import evaluator_liver as ev
    _write_dataset(tmp_path, n_cases=4, depth=7)
    (tmp_path / "k_folds.txt").write_text("Fold 0:0 1\nFold 1:2 3\n")
    args = t.make_args(batch_size=4, im_height=32, im_width=32, im_channel=3, test_fold=1, filter_size=0, noise_scale=0.05,
                       zoom_scale=(1.0, 1.2), random_flip=3, liver_percent=0.66, tumor_percent=0.5, eval_per_epoch=True,
                       eval_num_batches_per_epoch=2, model="UNet", log_step=1, eval_3d=True, use_global_dice=use_global_dice,
                       metrics_eval=["Dice", "VOE", "RVD", "ASSD", "RMSD", "MSD"])
    params = {"args": args, "model": UNet, "model_kwargs": dict(t.YML), "model_args": (), "solver": Solver(args),
              "solver_kwargs": {}, "lits_root": str(tmp_path)}
    e = est.CustomEstimator(models.model_fn, str(tmp_path / "run"), est.RunConfig(model_dir=str(tmp_path / "run"),
                                                                                 save_checkpoints_steps=0), params)
    e.train(lits.input_fn, steps=2)
    res = {}
    for on in ("host", "device"):
        res[on] = ev.get_evaluator("Volume", estimator=e, model_dir=str(tmp_path / "run"), params=params,
                                   metrics_on=on).run_with_session(None)
    _assert_results_match(res["device"], res["host"])


# ------------------------------------------------------------------------------------------------ LiTS-sized case
def test_lits_sized_case_largest_component_and_overlap_metrics():
    from boxsegliver_amd import loss_metrics, ops
    D, H, W = 450, 512, 512
    z, y, x = np.ogrid[:D, :H, :W]
    liver = ((z - 220) / 150.0) ** 2 + ((y - 250) / 120.0) ** 2 + ((x - 230) / 140.0) ** 2 <= 1.0
    rng = np.random.default_rng(0)
    pred = liver.copy()
    specks = rng.integers(0, [D, H, W], size=(4000, 3))
    pred[specks[:, 0], specks[:, 1], specks[:, 2]] = True
    ref = (((z - 224) / 148.0) ** 2 + ((y - 247) / 121.0) ** 2 + ((x - 233) / 139.0) ** 2 <= 1.0)
    p_dev, r_dev = _dev(pred.view(np.uint8)), _dev(ref.view(np.uint8))
    torch.cuda.synchronize()
    ops.largest_component3d(p_dev)                                          # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lc = ops.largest_component3d(p_dev)
    torch.cuda.synchronize()
    t_lc = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev = loss_metrics.metric_3d_device(lc, r_dev, required=["Dice", "VOE", "RVD"])
    t_m = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev_all = loss_metrics.metric_3d_device(lc, r_dev)
    t_all = time.perf_counter() - t0
    host_lc = _host_lc(pred)
    np.testing.assert_array_equal(lc.cpu().numpy(), host_lc)
    host = loss_metrics.metric_3d(host_lc, ref, required=["Dice", "VOE", "RVD"])
    assert dev == host
    assert set(dev_all) == {"Dice", "VOE", "RVD", "ASSD", "RMSD", "MSD"} and dev_all["MSD"] > 0
    print("\nLiTS-sized 450x512x512 on the device: largest component {:.1f} ms, Dice/VOE/RVD {:.1f} ms, "
          "all six metrics {:.1f} ms".format(t_lc * 1e3, t_m * 1e3, t_all * 1e3))
