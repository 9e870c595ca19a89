"""GPU: `unetk_lits_batch` (csrc/lits.hip, lits_batch_kernel) at full-slice coordinates and at its edges, on the case table of
lits_batch_cases.py (whose docstring describes the stores, the two references and derives the image bound;
test_lits_batch_host.py proves on the CPU that every row reaches what it is listed for).

  groups       labels equal R32 and R64 exactly; images within the derived bound of R32 and within the row's own
               max |R32 - R64| plus that bound of R64; C in {1, 3, 8}; flips, padding slices, slice indices of n_slices and
               2^31 - 1 in every group
  lab_scale    64, 1, 100 and 255 over a label slice that holds every value 0 .. 255
  clamp        boxes outside the slice read the box as the four min / max lines of the kernel clamp it.  The requests stay
               within a few rows of the slice and every store of this module lies between poisoned guards of at least
               guardbuf.GUARD_MIN_BYTES, so that even a missed clamp reads inside the allocation (and shows as a wrong value).
               Extreme int32 offsets and extents are NOT run: that they cannot leave the slice is read from those four lines
               (off in [0, src - 1], extent in [1, src - off]; max / min of int32 values, no arithmetic that could overflow
               before the clamp)
  second trip  one sample of 4097 x 4096 = 2^24 + 4096 pixels: the grid is capped at 65,536 blocks of 256, so the pixels from
               2^24 on are written by the second trip of the grid-stride loop; image, label and noise counters there
  hi == lo     NaN exactly where R32 gives NaN (every real slice), padding slices exactly 0, labels as ever: documents the
               behaviour, asks for nothing
  noise        the kernel's counter generator restated in uint64 (lits_batch_cases.u01): noisy == clean + (2 u - 1) * scale
               at counter i * C + c to one float32 ulp of the sum, exactly clean on padding slices, different between channels
               and samples.  A counter truncated to 32 bits would first differ at 2^32 output values (16 GiB): not run
  C entry      guard bands around images and labels, inputs bit-equal, every refusal before any launch
  guide        `unetk_lits_spatial_guide` repeats the clamp, flip and tap lines: the same tables, against
               test_lits_guide_host.render_numpy at that suite's bound of 2e-6

Figures (MI355X; the bound is 12 e / (hi - lo) + 2^-24 with e = 2^-10 raw units on the big store, 2^-14 on the small one):
  group        bound      max |R32 - R64|   kernel: max |got - R32|   max |got - R64|
  ws256        4.5e-7     6.1e-5            2.4e-7                    6.1e-5
  up512x384    4.5e-7     2.7e-5            2.4e-7                    2.7e-5
  floor64      4.5e-7     6.2e-5            1.8e-7                    6.2e-5
  over22x24    4.5e-7     4.1e-5            1.2e-7                    4.1e-5
  under8x15    4.5e-7     6.2e-5            1.8e-7                    6.2e-5
  tie33, tie9  2.2e-6     2.9e-8            0                         2.9e-8
  one1x1       2.2e-6     2.4e-8            0                         2.4e-8
  one1x13      2.2e-6     2.9e-6            3.6e-7                    2.7e-6
  one31x1      2.2e-6     2.1e-6            3.6e-7                    2.1e-6
  clamp        1.9e-6     2.6e-6            3.6e-7                    2.6e-6
  second trip  1.9e-6     7.4e-7            6.6e-7                    6.5e-7
(the maxima over C = 1, 3, 8 and over a group's rows).  On the CPU, R32 with fused lerps differs from R32 by at most 2.4e-7 on the
full-slice rows, the reciprocal-multiply coordinate by 3.2e-5 .. 1.2e-4 and the fma weight by 1.6e-5 .. 3.1e-5: 35 to 280 times
the bound.  Noise: at most 0.50 of the one-ulp tolerance on every seed, the second trip included.  Guide: at most 1.2e-7.

Each of these, reverted alone in lits_batch_kernel in a scratch build, fails the rows named (and passes every other test here):
  roundf -> rintf in the nearest tap       the tie33, tie9, one1x13 and one31x1 groups, every lab_scale row, the second trip
  i1 = i0 + 1 without the clamp            the over22x24 group (i0 is the last pixel there, f = 3e-5)
  no left-right flip                       every group but one1x1 and one31x1, the lab_scale and clamp rows
  a doubled grid-stride increment          both second-trip tests, which name the pixels from index 2^24 on
  the noise counter i instead of i*C + c   test_noise_is_the_counter_generator at C = 3, every seed
"""
import ctypes

import numpy as np
import pytest
import torch

import lits_batch_cases as lc
from guardbuf import GUARD_MIN_BYTES, Guarded
from test_lits_guide_host import render_numpy

pytestmark = pytest.mark.gpu

GROUP_C = [(g.name, c) for g in lc.GROUPS for c in lc.CHANNELS]
_DEV = {}


class _DeviceStore(object):
    """A store on the device, each of its two arrays between poisoned guards (all bits set) of GUARD_MIN_BYTES or more."""

    def __init__(self, name):
        im, lb = lc.store(name)
        self.views, self.flats = [], []
        for a, dt in ((im.view(np.int16), torch.int16), (lb, torch.uint8)):
            guard = (GUARD_MIN_BYTES // a.itemsize + 127) // 128 * 128
            flat = torch.full((2 * guard + a.size,), -1 if dt == torch.int16 else 255, dtype=dt, device="cuda")
            flat[guard:guard + a.size].copy_(torch.from_numpy(np.array(a)).reshape(-1))
            self.flats.append(flat)
            self.views.append(flat[guard:guard + a.size].view(a.shape))
        self.snaps = [f.clone() for f in self.flats]

    def unchanged(self):
        return all(torch.equal(f, s) for f, s in zip(self.flats, self.snaps))


def _store(name):
    if name not in _DEV:
        _DEV[name] = _DeviceStore(name)
    return _DEV[name]


def _call(desc, ptrs):
    """unetk_lits_batch through the C ABI: ptrs = slices, label slices, table, clip, images, labels (None = NULL)."""
    from boxsegliver_amd import _abi
    args = [None if desc is None else ctypes.byref(desc)] + [None if p is None else ctypes.c_void_p(p) for p in ptrs]
    return _abi.lib().unetk_lits_batch(*(args + [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]))


def _run(store_name, rows, out_hw, lab_scale=lc.LB_SCALE, noise_scale=0.0, seed=0):
    """One call on a device store; the outputs start as NaN / -12345, so an element the kernel never wrote cannot pass for a
    value that an earlier call left in recycled memory."""
    from boxsegliver_amd import _abi
    st = _store(store_name)
    tab, clip = lc.table(rows)
    tab_t, clip_t = torch.from_numpy(tab).cuda(), torch.from_numpy(clip).cuda()
    n, c, (h, w) = len(rows), len(rows[0].chans), out_hw
    images = torch.full((n, h, w, c), float("nan"), dtype=torch.float32, device="cuda")
    labels = torch.full((n, h, w), -12345, dtype=torch.int32, device="cuda")
    src_n, src_h, src_w = st.views[0].shape
    d = _abi.LitsDesc(n, h, w, c, src_n, src_h, src_w, int(lab_scale), int(seed), float(noise_scale))
    rc = _call(d, [t.data_ptr() for t in (st.views[0], st.views[1], tab_t, clip_t, images, labels)])
    torch.cuda.synchronize()
    assert rc == 0
    assert st.unchanged() and np.array_equal(tab_t.cpu().numpy(), tab) and np.array_equal(clip_t.cpu().numpy(), clip)
    return images.cpu().numpy(), labels.cpu().numpy()


def _real(store_name, rows):
    """bool [N, 1, 1, C]: the channel reads a slice of the store (anything else is a padding slice)."""
    n = lc.STORES[store_name].n
    return np.array([[0 <= s < n for s in r.chans] for r in rows])[:, None, None, :]


def _check_rows(store_name, rows, out_hw, got_img, got_lab, lab_scale=lc.LB_SCALE, what=""):
    """Every row against both references; returns (bound, gap, err32, err64) maxima over the rows."""
    fig = np.zeros(4)
    for j, r in enumerate(rows):
        tag = "{} row {} {}".format(what, j, r)
        img32, lab32 = lc.r32_sample(store_name, r, out_hw, lab_scale)
        img64, lab64 = lc.r64_sample(store_name, r, out_hw, lab_scale)
        np.testing.assert_array_equal(got_lab[j], lab32, err_msg=tag)
        np.testing.assert_array_equal(got_lab[j], lab64, err_msg=tag)
        bound = lc.image_bound(store_name, r.clip)
        gap = float(np.abs(img32 - img64).max())
        e32 = float(np.abs(got_img[j].astype(np.float64) - img32).max())
        e64 = float(np.abs(got_img[j] - img64).max())
        fig = np.maximum(fig, [bound, gap, e32, e64])
        assert e32 <= bound, "{}: |got - R32| {:.3e} > bound {:.3e}".format(tag, e32, bound)
        assert e64 <= gap + bound, "{}: |got - R64| {:.3e} > gap {:.3e} + bound {:.3e}".format(tag, e64, gap, bound)
    return fig


@pytest.mark.parametrize("name,channels", GROUP_C)
def test_group_matches_both_references(name, channels):
    g = lc.GROUP[name]
    rows = lc.rows_of(name, channels)
    img, lab = _run(g.store, rows, g.out_hw)
    assert img.shape == (len(rows),) + g.out_hw + (channels,) and lab.shape == (len(rows),) + g.out_hw
    assert np.all(np.broadcast_to(~_real(g.store, rows), img.shape) <= (img == 0))          # padding slices: exactly 0
    fig = _check_rows(g.store, rows, g.out_hw, img, lab, what=name)
    print("FIG {:<10} C={} bound {:.2e}  R32-R64 {:.2e}  got-R32 {:.2e}  got-R64 {:.2e}".format(name, channels, *fig))


@pytest.mark.parametrize("lab_scale", lc.LAB_SCALES)
def test_lab_scale_over_every_label_value(lab_scale):
    rows = lc.lab_scale_rows()
    img, lab = _run("small", rows, lc.LAB_SCALE_OUT_HW, lab_scale)
    _check_rows("small", rows, lc.LAB_SCALE_OUT_HW, img, lab, lab_scale, "lab_scale {}".format(lab_scale))
    assert lab[0].max() == 255 // lab_scale and len(np.unique(lab[0])) == 255 // lab_scale + 1


@pytest.mark.parametrize("channels", [1, 3])
def test_boxes_outside_the_slice_read_the_clamped_box(channels):
    rows = lc.clamp_rows(channels)
    img, lab = _run("small", rows, lc.CLAMP_OUT_HW)
    fig = _check_rows("small", rows, lc.CLAMP_OUT_HW, img, lab, what="clamp")
    assert np.isfinite(img).all() and img.max() <= 1.0                        # no poison (65535) reached the lerp
    print("FIG clamp      C={} bound {:.2e}  R32-R64 {:.2e}  got-R32 {:.2e}  got-R64 {:.2e}".format(channels, *fig))


# ------------------------------------------------------------------------------------------------- the second loop trip
def _name_pixels(bad, w):
    flat = np.flatnonzero(bad.reshape(-1)) if bad.ndim == 2 else np.flatnonzero(bad.reshape(bad.shape[0] * bad.shape[1], -1).any(axis=1))
    late = flat[flat >= 1 << 24]
    return "{} pixels differ, {} of them at index >= 2^24 (second loop trip); first {} = (y {}, x {}){}".format(
        len(flat), len(late), int(flat[0]), int(flat[0]) // w, int(flat[0]) % w,
        "" if not len(late) else "; first late one {} = (y {}, x {})".format(int(late[0]), int(late[0]) // w, int(late[0]) % w))


def test_second_loop_trip_image_and_label():
    h, w = lc.TRIP2_HW
    img, lab = _run("small", (lc.TRIP2_ROW,), lc.TRIP2_HW)
    img, lab = img[0], lab[0]
    img32, lab32 = lc.r32_sample("small", lc.TRIP2_ROW, lc.TRIP2_HW)
    bad = lab != lab32
    assert not bad.any(), "label vs R32: " + _name_pixels(bad, w)
    bound = lc.image_bound("small", lc.TRIP2_ROW.clip)
    err = np.abs(img - img32)
    assert float(err.max()) <= bound, "image vs R32 (bound {:.2e}, max {:.2e}): ".format(bound, err.max()) + _name_pixels(
        err > bound, w)
    e32 = float(err.max())
    del err
    img64, lab64 = lc.r64_sample("small", lc.TRIP2_ROW, lc.TRIP2_HW)
    bad = lab != lab64
    assert not bad.any(), "label vs R64: " + _name_pixels(bad, w)
    gap = float(np.abs(img32 - img64).max())
    err = np.abs(img - img64)
    assert float(err.max()) <= gap + bound, "image vs R64 (gap {:.2e}): ".format(gap) + _name_pixels(err > gap + bound, w)
    assert len(np.unique(lab[-1])) > 1 and img[-1].std() > 0.1                 # the last row, all of it late, is not flat
    print("FIG trip2      C=1 bound {:.2e}  R32-R64 {:.2e}  got-R32 {:.2e}  got-R64 {:.2e}".format(bound, gap, e32,
                                                                                                    float(err.max())))


def test_second_loop_trip_noise_counters():
    clean, lab0 = _run("small", (lc.TRIP2_ROW,), lc.TRIP2_HW)
    noisy, lab1 = _run("small", (lc.TRIP2_ROW,), lc.TRIP2_HW, noise_scale=0.05, seed=0xFFFFFFFF)
    assert np.array_equal(lab0, lab1)
    worst = lc.check_noise(noisy, clean, 0xFFFFFFFF, 0.05, True, "second trip (flat elements >= 2^24 are its pixels)")
    late = (noisy - clean)[0].reshape(-1)[1 << 24:]
    assert late.std() > 0.02 and len(np.unique(late)) > 4000                   # 4096 late pixels, each its own draw
    print("FIG trip2 noise: max error {:.2f} of the tolerance".format(worst))


# ------------------------------------------------------------------------------------------------- noise, window of zero width
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("seed", lc.NOISE_SEEDS)
def test_noise_is_the_counter_generator(seed, channels):
    g = lc.GROUP["tie33"]
    rows = lc.rows_of("tie33", channels)
    real = _real(g.store, rows)
    clean, lab0 = _run(g.store, rows, g.out_hw)
    noisy, lab1 = _run(g.store, rows, g.out_hw, noise_scale=0.05, seed=seed)
    assert np.array_equal(lab0, lab1)
    worst = lc.check_noise(noisy, clean, seed, 0.05, real, "seed {} C {}".format(seed, channels))
    d = noisy - clean
    assert np.all(np.abs(d) <= 0.05 + 1e-6)
    assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[2], d[3])                # samples draw their own noise
    if channels > 1:
        assert not np.array_equal(d[1, ..., 0], d[1, ..., 1]) and not np.array_equal(d[1, ..., 1], d[1, ..., 2])
    print("FIG noise seed {} C={}: max error {:.2f} of the tolerance".format(seed, channels, worst))


def test_window_of_zero_width_gives_nan_where_r32_does():
    g = lc.GROUP["tie9"]
    rows = tuple(r._replace(clip=(lc.F32(1200), lc.F32(1200))) for r in lc.rows_of("tie9", 3))
    real = np.broadcast_to(_real(g.store, rows), (len(rows),) + g.out_hw + (3,))
    img, lab = _run(g.store, rows, g.out_hw)
    want_img, want_lab = lc.r32_batch(g.store, rows, g.out_hw)
    assert np.array_equal(np.isnan(img), np.isnan(want_img)) and np.array_equal(np.isnan(img), real)
    assert np.all(img[~real] == 0) and (~real).any()
    np.testing.assert_array_equal(lab, want_lab)


# ------------------------------------------------------------------------------------------------- the C entry
@pytest.mark.parametrize("name,channels", [("tie9", 3), ("one1x1", 8), ("over22x24", 1)])
def test_guard_bands_and_refusals(name, channels):
    """Every image and label element is written, nothing outside them changes, the inputs stay bit-equal; every malformed call
    is refused with a non-zero code before any launch and leaves the outputs untouched."""
    from boxsegliver_amd import _abi
    g = lc.GROUP[name]
    st = _store(g.store)
    rows = lc.rows_of(name, channels)
    n, (h, w), (src_n, src_h, src_w) = len(rows), g.out_hw, st.views[0].shape
    tab, clip = lc.table(rows)
    tab_t = torch.zeros((n, 16), dtype=torch.int32, device="cuda").reshape(-1)       # room for the refused C = 9 call's rows
    tab_t[:tab.size].copy_(torch.from_numpy(tab).reshape(-1))
    clip_t = torch.from_numpy(clip).cuda()
    snaps = [tab_t.clone(), clip_t.clone()]
    images = Guarded((n, h, w, channels))
    labels = Guarded((n, h, w, 1))                                                   # int32 labels in float32 storage
    fields = dict(N=n, H=h, W=w, C=channels, n_slices=src_n, src_h=src_h, src_w=src_w, lab_scale=lc.LB_SCALE, seed=5, noise_scale=0.0)
    ptrs = [st.views[0].data_ptr(), st.views[1].data_ptr(), tab_t.data_ptr(), clip_t.data_ptr(), images.ptr(), labels.ptr()]
    rc = _call(_abi.LitsDesc(**fields), ptrs)
    torch.cuda.synchronize()
    assert rc == 0
    assert images.unwritten() == 0 and labels.unwritten() == 0 and images.check_untouched() and labels.check_untouched()
    assert st.unchanged() and torch.equal(tab_t, snaps[0]) and torch.equal(clip_t, snaps[1])
    _check_rows(g.store, rows, g.out_hw, images.view.cpu().numpy(), labels.view.view(torch.int32)[..., 0].cpu().numpy(), what=name)
    images.reset()
    labels.reset()
    refused = [("NULL descriptor", None, ptrs)]
    refused += [("NULL pointer {}".format(k), fields, ptrs[:k] + [None] + ptrs[k + 1:]) for k in range(6)]
    refused += [("{} = {}".format(f, v), dict(fields, **{f: v}), ptrs) for f in ("N", "H", "W", "C", "src_h", "src_w") for v in (0, -1)]
    refused += [("C = 9", dict(fields, C=9), ptrs), ("lab_scale = 0", dict(fields, lab_scale=0), ptrs),
                ("lab_scale = -64", dict(fields, lab_scale=-64), ptrs)]
    for what, f, p in refused:
        assert _call(None if f is None else _abi.LitsDesc(**f), p) != 0, what
    torch.cuda.synchronize()
    assert images.changed_anywhere() == 0 and labels.changed_anywhere() == 0
    assert st.unchanged() and torch.equal(tab_t, snaps[0]) and torch.equal(clip_t, snaps[1])


# ------------------------------------------------------------------------------------------------- the guide on the same tables
def _objects(rng, rows, src_hw):
    counts = [(2, 0, 3, 1, 4)[j % 5] for j in range(len(rows))]
    objs = []
    for r, k in zip(rows, counts):
        _, _, ch, cw = lc.clamp_box(r.box, src_hw)
        cen = np.stack([rng.uniform(-4, ch + 4, k), rng.uniform(-4, cw + 4, k)], axis=1)
        sd = rng.choice([0.0, 0.3, 1.0, 2.5, 7.0, 60.0], size=(k, 2))
        objs.append(np.concatenate([cen, sd], axis=1))
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32), np.concatenate(objs).astype(np.float32).reshape(-1, 4)


@pytest.mark.parametrize("name", ["ws256", "floor64", "clamp"])
def test_guide_kernel_on_the_same_tables(name):
    from boxsegliver_amd import ops
    if name == "clamp":
        rows, out_hw, src_hw = lc.clamp_rows(3), lc.CLAMP_OUT_HW, lc.STORES["small"].hw
    else:
        rows, out_hw, src_hw = lc.rows_of(name, 3), lc.GROUP[name].out_hw, lc.STORES[lc.GROUP[name].store].hw
    tab, _ = lc.table(rows)
    ptr, obj = _objects(np.random.default_rng(len(rows)), rows, src_hw)
    got = ops.lits_spatial_guide(torch.from_numpy(tab).cuda(), torch.from_numpy(ptr).cuda(), torch.from_numpy(obj).cuda(), out_hw, 3,
                                 src_hw, 1.0).cpu().numpy()
    want = render_numpy(tab, ptr, obj, out_hw, 3, src_hw)
    assert got.shape == (len(rows),) + tuple(out_hw) + (1,)
    for j in range(len(rows)):
        np.testing.assert_allclose(got[j], want[j], rtol=0, atol=2e-6, err_msg="{} row {} {}".format(name, j, rows[j]))
        assert (ptr[j + 1] > ptr[j]) or np.all(got[j] == np.float32(0.5))
    assert max(float(got[j].max()) for j in range(len(rows))) > 0.75                  # the guides are not flat
    print("FIG guide {}: max |got - render_numpy| {:.2e}".format(name, float(np.abs(got - want).max())))
