"""GPU: hard-negative training of `liver_3d` -- `unetk_fp_mask3d` (csrc/evalvol.hip),
`unetk_lits_pick_voxel_rows` (csrc/lits3d.hip) and `unetk_lits3d_clicks_neg` (csrc/lits3d_clicks.hip) through the C ABI in guarded
buffers, against the restatements of hard_neg_ref.py and what the reference itself gave (tests/golden/ref_clicks3d_neg.json); and
the flags end to end on the tiny LiTS root of the 3-D tests: mine, load the plane, train."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import click3d_shapes as c3
import guardbuf
import hard_neg_ref as hn
import lits3d_clicks_ref as cref
import lits3d_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LARGE = (6, 32, 40)
REF_CLICKS, SMALL_CLICKS, LAST = c3.REF_CLICKS, c3.SMALL_CLICKS, c3.LAST
BYTE_GUARD = 1 << 16


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _i32(g):
    return g.view.view(torch.int32)


# ------------------------------------------------------------------------------------------------- unetk_fp_mask3d
def _serpentine(shape, z):
    """One 1-voxel-wide path that runs along every second row of slice z and turns at alternating ends."""
    m = np.zeros(shape, np.uint8)
    for j, y in enumerate(range(0, shape[1], 2)):
        m[z, y, :] = 1
        if y + 1 < shape[1] and y + 2 < shape[1]:
            m[z, y + 1, shape[2] - 1 if j % 2 == 0 else 0] = 1
    return m


def _mining_volumes():
    """name -> (pred in {0, 1, 2}, lab in {0, 1, 2})"""
    out = {}
    pred = np.zeros((6, 12, 16), np.uint8)
    lab = np.zeros_like(pred)
    pred[0, 0, 0:6] = 2                      # 6 voxels: kept at min_size 6
    pred[1, 3, 0:5] = 2                      # 5 voxels: dropped
    pred[2, 0:3, 8:10] = 2                   # 6 voxels, exactly ONE on the labelled tumour: dropped
    lab[2, 2, 9] = 2
    pred[4, 2, 2] = pred[4, 3, 3] = 2        # touch only diagonally: two components
    pred[4, 5, 15] = pred[4, 6, 0] = 2       # x = W - 1 next to x = 0 of the following row: not connected
    pred[3:6, 10, 5] = 2                     # spans slices, with ...
    pred[5, 10, 6:9] = 2                     # ... an L of 6
    pred[0:2, 6:9, 12:15] = 1                # liver-valued, 18 voxels, on labelled liver: no tumour component at label 2
    lab[0:2, 5:10, 11:16] = 1
    pred[3, 0:3, 0:3] = 1                    # liver-valued, 9 voxels, on nothing: a false positive at label 1 only
    out["small"] = (pred, lab)
    out["empty"] = (np.zeros((6, 12, 16), np.uint8), lab.copy())
    # 9 x 40 x 70 = 25 200 voxels, 99 blocks: a serpentine through slice 4 (1 419 voxels, root in the first row, members in
    # blocks far apart), random blobs of both classes above and below it, some of them on the labels
    rng = np.random.default_rng(5)
    big = (9, 40, 70)
    pred = _serpentine(big, 4) * 2
    pred[0:3][rng.random((3,) + big[1:]) < 0.30] = 2
    pred[6:9][rng.random((3,) + big[1:]) < 0.55] = 1
    pred[7, :, 69] = 1
    pred[8, :, 0] = 1
    lab = np.zeros(big, np.uint8)
    lab[1, 10:20, 10:30] = 2
    lab[7, 0:30, 0:35] = 1
    out["large"] = (pred.astype(np.uint8), lab)
    # only the serpentine's LAST voxel lies on the label: the whole path is dropped
    pred2 = (_serpentine(big, 4) * 2).astype(np.uint8)
    lab2 = np.zeros(big, np.uint8)
    ys, xs = np.nonzero(pred2[4])
    lab2[4, ys[-1], xs[-1]] = 2
    out["serpentine_hit"] = (pred2, lab2)
    return out


MINING = _mining_volumes()


def _fp_call(pred, lab, pred_label, obj_label, min_size, out_value, ws_bytes=None, nulls=(), dims=None):
    """unetk_fp_mask3d through the C ABI with every output in a guarded buffer -> (code, out, slice_counts, head) as numpy, None
    where the call was refused (then nothing may have been written)."""
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    d, h, w = pred.shape if dims is None else dims
    n = int(np.prod(pred.shape))
    dp = torch.from_numpy(pred).cuda()
    dl = torch.from_numpy((lab * ref.LB_SCALE).astype(np.uint8)).cuda()
    flat = torch.full((2 * BYTE_GUARD + n,), 0xA5, dtype=torch.uint8, device="cuda")
    counts, head = guardbuf.guarded((pred.shape[0],)), guardbuf.guarded((4,))
    nbytes = int(lib.unetk_fp_mask3d_ws_bytes(*pred.shape))
    assert nbytes == 2 * ((4 * n + 255) & ~255)
    ws = guardbuf.GuardedWorkspace(nbytes)
    ws.fill(0xFF)
    ptrs = dict(pred=dp.data_ptr(), lab=dl.data_ptr(), out=flat.data_ptr() + BYTE_GUARD, counts=counts.ptr(), head=head.ptr(),
                ws=ws.ptr())
    for name in nulls:
        ptrs[name] = 0
    code = lib.unetk_fp_mask3d(ctypes.c_void_p(ptrs["pred"]), ctypes.c_void_p(ptrs["lab"]), d, h, w, pred_label, ref.LB_SCALE, obj_label,
                               min_size, out_value, ctypes.c_void_p(ptrs["out"]), ctypes.c_void_p(ptrs["counts"]),
                               ctypes.c_void_p(ptrs["head"]), ctypes.c_void_p(ptrs["ws"]), nbytes if ws_bytes is None else ws_bytes,
                               _abi.stream_ptr())
    torch.cuda.synchronize()
    assert counts.check_untouched() and head.check_untouched() and ws.guard_intact()
    assert bool((flat[:BYTE_GUARD] == 0xA5).all()) and bool((flat[BYTE_GUARD + n:] == 0xA5).all())
    if code != 0:                                                                     # refused: nothing launched
        assert bool((flat == 0xA5).all()) and counts.changed_anywhere() == 0 and head.changed_anywhere() == 0
        return code, None, None, None
    assert counts.unwritten() == 0 and head.unwritten() == 0
    return (code, flat[BYTE_GUARD:BYTE_GUARD + n].view(pred.shape).cpu().numpy(), _i32(counts).cpu().numpy(),
            _i32(head).cpu().numpy().tolist())


@pytest.mark.parametrize("name", sorted(MINING))
@pytest.mark.parametrize("label", [1, 2])
def test_fp_mask3d_equals_the_restatement(name, label):
    pred, lab = MINING[name]
    for min_size, out_value in ((6, 64), (1, 1), (7, 255)):
        want_out, want_counts, want_head = hn.fp_mask(pred, lab, label, label, min_size, out_value)
        code, out, counts, head = _fp_call(pred, lab, label, label, min_size, out_value)
        assert code == 0
        assert head == want_head, (name, label, min_size)
        np.testing.assert_array_equal(counts, want_counts)
        np.testing.assert_array_equal(out, want_out)                                  # every voxel written: no 0xA5 is left
        again = _fp_call(pred, lab, label, label, min_size, out_value)                # two calls give identical bits
        assert again[3] == head and np.array_equal(again[1], out) and np.array_equal(again[2], counts)
    # what the volumes are there for
    at6 = hn.fp_mask(pred, lab, label, label, 6)
    if name == "small" and label == 2:
        assert at6[2] == [8, 2, 12, 0]                                                # the row of 6 and the L across slices
        assert hn.fp_mask(pred, lab, 2, 2, 5)[2][1] == 3 and at6[0][2, 0:3, 8:10].sum() == 0
    if name == "small" and label == 1:
        assert at6[0][3, 0:3, 0:3].all() and not at6[0][0:2, 6:9, 12:15].any()
    if name == "empty":
        assert at6[2] == [0, 0, 0, 0]
    if name == "large" and label == 2:
        assert at6[0][4].sum() == _serpentine(pred.shape, 4).sum() > 256 * 5          # the serpentine is kept whole
    if name == "serpentine_hit":
        assert at6[2] == [1, 0, 0, 0]


def test_fp_mask3d_through_ops():
    from boxsegliver_amd import ops
    pred, lab = MINING["large"]
    dp, dl = torch.from_numpy(pred).cuda(), torch.from_numpy((lab * ref.LB_SCALE).astype(np.uint8)).cuda()
    out, counts, head = ops.fp_mask3d(dp, dl, 2, 2, min_size=6, out_value=ref.LB_SCALE)
    want = hn.fp_mask(pred, lab, 2, 2, 6, ref.LB_SCALE)
    np.testing.assert_array_equal(out.cpu().numpy(), want[0])
    assert counts.dtype == torch.int32 and counts.cpu().numpy().tolist() == want[1].tolist() and head.tolist() == want[2]


def test_fp_mask3d_refusals_leave_the_outputs_untouched():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    pred, lab = MINING["small"]
    n = pred.size
    for name in ("pred", "lab", "out", "counts", "head", "ws"):
        assert _fp_call(pred, lab, 2, 2, 6, 1, nulls=(name,))[0] == -1, name         # UNETK_E_BADARG
    for dims in ((0, 12, 16), (6, 0, 16), (6, 12, 0), (-1, 12, 16)):
        assert _fp_call(pred, lab, 2, 2, 6, 1, dims=dims)[0] == -1
        assert lib.unetk_fp_mask3d_ws_bytes(*dims) == 0
    for args in ((0, 2, 6, 1), (2, 0, 6, 1), (2, 2, 0, 1), (2, 2, 6, 0), (2, 2, 6, 256)):
        assert _fp_call(pred, lab, *args)[0] == -1
    assert _fp_call(pred, lab, 2, 2, 6, 1, dims=(2048, 1024, 1024))[0] == -2         # UNETK_E_UNSUPPORTED: 2^31 voxels, no launch
    assert lib.unetk_fp_mask3d_ws_bytes(2048, 1024, 1024) == 0 and lib.unetk_fp_mask3d_ws_bytes(2047, 1024, 1024) > 0
    full = 2 * ((4 * n + 255) & ~255)
    assert _fp_call(pred, lab, 2, 2, 6, 1, ws_bytes=full - 1)[0] == -3               # UNETK_E_WORKSPACE
    assert _fp_call(pred, lab, 2, 2, 6, 1, ws_bytes=full)[0] == 0


# ------------------------------------------------------------------------------------------------- unetk_lits_pick_voxel_rows
@pytest.fixture(scope="module")
def store():
    cases = ref.make_cases()
    im, lb, base = ref.stack_store(cases)
    neg = hn.store_neg()
    plane = np.concatenate(neg) * np.uint8(ref.LB_SCALE)
    return dict(cases=cases, base=base, neg=neg, im=torch.from_numpy(im.view(np.int16)).cuda(), lb=torch.from_numpy(lb).cuda(),
                plane=torch.from_numpy(plane).cuda())


def test_pick_voxel_rows_serves_its_own_rows_only(store):
    from boxsegliver_amd import ops
    cases, base, neg = store["cases"], store["base"], store["neg"]
    rows, want_neg, want_lab = [], [], []
    for ci, z in ((0, 2), (0, 3), (0, 9), (1, 4), (3, 0), (3, 8)):
        pos = np.argwhere(neg[ci][z])
        for k in sorted({0, len(pos) - 1, len(pos) // 2}):
            rows.append(ref.table_row(base[ci], ref.DEPTHS[ci], (z, 33, 44), (16, 20), forced=2, k=k))
            want_neg.append(pos[k])
            want_lab.append((33, 44))
    for ci, z in ((0, 7), (3, 2)):                                                    # rows of the label plane, and uniform rows
        pos = np.argwhere(cases[ci][1][z] >= 2)
        rows.append(ref.table_row(base[ci], ref.DEPTHS[ci], (z, 30, 41), (16, 20), forced=1, k=len(pos) - 1))
        want_neg.append((30, 41))
        want_lab.append(pos[-1])
        rows.append(ref.table_row(base[ci], ref.DEPTHS[ci], (z, 31, 7), (16, 20), forced=0, k=3))
        want_neg.append((31, 7))
        want_lab.append((31, 7))
    host = np.stack(rows)
    other = [c for c in range(16) if c not in (3, 4)]
    tab, status = torch.from_numpy(host).cuda(), _status()
    ops.lits_pick_voxel_rows(store["plane"], tab, 2, status, 1)                       # value 2 on the neg plane
    np.testing.assert_array_equal(tab[:, 3:5].cpu().numpy(), np.array(want_neg))
    assert torch.equal(tab[:, other].cpu(), torch.from_numpy(host[:, other])) and int(status.item()) == 0
    tab = torch.from_numpy(host).cuda()
    ops.lits_pick_voxel_rows(store["lb"], tab, 1, status, 2)                          # value 1 on the label plane
    np.testing.assert_array_equal(tab[:, 3:5].cpu().numpy(), np.array(want_lab))
    assert int(status.item()) == 0
    # both calls, as a batch makes them: every row has its centre
    ops.lits_pick_voxel_rows(store["plane"], tab, 2, status, 1)
    both = np.where((host[:, 11] == 2)[:, None], np.array(want_neg), np.array(want_lab))
    np.testing.assert_array_equal(tab[:, 3:5].cpu().numpy(), both)
    # a table without value 2 rows: the new entry with value 1 and the existing entry give the same table
    plain = host[host[:, 11] != 2]
    a, b = torch.from_numpy(plain).cuda(), torch.from_numpy(plain).cuda()
    ops.lits_pick_voxels(store["lb"], a, 2, status)
    ops.lits_pick_voxel_rows(store["lb"], b, 1, status, 2)
    assert torch.equal(a, b) and int(status.item()) == 0 and not torch.equal(a.cpu(), torch.from_numpy(plain))


def test_pick_voxel_rows_flags_a_rank_beyond_the_count(store):
    from boxsegliver_amd import _abi, ops
    from boxsegliver_amd.data import lits3d
    base, neg = store["base"], store["neg"]
    n2 = int(neg[0][2].sum())
    bad = [ref.table_row(base[0], 12, (2, 9, 9), (16, 20), forced=2, k=n2),           # one past the last rank
           ref.table_row(base[0], 12, (5, 9, 9), (16, 20), forced=2, k=0),            # a slice without a false positive
           ref.table_row(base[0], 12, (2, 9, 9), (16, 20), forced=2, k=-1),
           ref.table_row(10 ** 6, 9, (4, 9, 9), (16, 20), forced=2, k=0)]             # a slice outside the store
    keep = [ref.table_row(base[0], 12, (2, 8, 7), (16, 20), forced=1, k=10 ** 6), ref.table_row(base[0], 12, (2, 6, 5), (16, 20))]
    for j, row in enumerate(bad):
        tab, status = torch.from_numpy(np.stack([row] + keep)).cuda(), _status()
        ops.lits_pick_voxel_rows(store["plane"], tab, 2, status, 1)
        word = int(status.item())
        assert word & 1 and word == 3, j                                              # the bit of the existing entry, and the plane's
        np.testing.assert_array_equal(tab[:, 3:5].cpu().numpy(), [[0, 0], [8, 7], [6, 5]])
        with pytest.raises(RuntimeError, match="`neg` plane"):
            lits3d.check_status(status, "test")
    tab, status = torch.from_numpy(np.stack(keep)).cuda(), _status()
    ops.lits_pick_voxel_rows(store["plane"], tab, 2, status, 1)
    assert int(status.item()) == 0
    ops.lits_pick_voxel_rows(store["lb"], tab, 1, status, 2)                          # the label plane's rows keep bit 0 alone
    assert int(status.item()) == 1
    lib = _abi.lib()
    for value in (0, -1):
        assert lib.unetk_lits_pick_voxel_rows(_abi.ptr(store["plane"]), *store["plane"].shape, 64, 1, _abi.ptr(tab), 2, _abi.ptr(status),
                                              value, _abi.stream_ptr()) == -1


# ------------------------------------------------------------------------------------------------- unetk_lits3d_clicks_neg
def _click_rows(n, seed):
    rng = np.random.default_rng(seed)
    tab = np.zeros((n, 12), np.uint32)
    tab[:, 0] = 4
    tab[:, 1] = 4
    tab[:, 2] = np.where(np.arange(n) % 2 == 0, 1, 3)
    tab[:, 4:] = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    tab[0::3, 4], tab[1::3, 5], tab[1::3, 8], tab[0::3, 9] = 0, LAST, 0, LAST
    tab[2::5, 0], tab[3::5, 1], tab[4::7, 1] = 2, 0, 1
    return tab


def _run(lb, plane, tab, rows, shape, params, obj_label=1):
    from boxsegliver_amd import ops
    ctab = torch.from_numpy(rows.view(np.int32)).cuda()
    status = _status()
    pts, cnt = ops.lits3d_clicks(lb, tab, ctab, shape, status, obj_label, params, neg_slices=plane)
    again = ops.lits3d_clicks(lb, tab, ctab, shape, status, obj_label, params, neg_slices=plane)
    assert torch.equal(pts, again[0]) and torch.equal(cnt, again[1])                  # two calls give identical bits
    return pts.cpu().numpy(), cnt.cpu().numpy(), int(status.item())


def _samples(shape, zoom):
    from boxsegliver_amd.data import lits3d
    crop = tuple(int(v) for v in lits3d.crop_shape(shape[1:], [zoom, zoom * 0.97 + 0.03]))
    d0 = ref.DEPTHS[0]
    out = [(0, c, crop) for c in [(0, 0, 0), (d0 - 1, ref.H - 1, ref.W - 1), (0, ref.H - 1, 0), (d0 - 1, 0, ref.W - 1)]]
    out += [(0, (3, 8, 9), crop), (0, (3, 23, 38), crop), (0, (9, 34, 6), crop), (1, (4, 13, 13), crop), (2, (2, 17, 21), crop),
            (2, (4, 39, 0), crop), (3, (1, 2, 3), crop), (3, (7, 36, 44), crop), (3, (4, 20, 24), crop)]
    return out


@pytest.mark.parametrize("shape,zoom", [((6, 16, 20), 1.0), ((6, 16, 20), 1.25), (LARGE, 1.125), (LARGE, 1.4)])
@pytest.mark.parametrize("params", [SMALL_CLICKS, REF_CLICKS])
def test_clicks_neg_equal_the_restatement(store, shape, zoom, params):
    samples = _samples(shape, zoom)
    tab = torch.from_numpy(np.stack([ref.table_row(store["base"][ci], ref.DEPTHS[ci], c, crop) for ci, c, crop in samples])).cuda()
    seen = dict(neg_rows=0, plain_rows=0, stopped=0, slices=0, on_object=0, shallow=0)
    for obj_label in (1, 2):
        rows = _click_rows(len(samples), 23 + obj_label)
        pts, cnt, status = _run(store["lb"], store["plane"], tab, rows, shape, params, obj_label)
        assert status == 0
        for j, (ci, c, crop) in enumerate(samples):
            obj, _ = cref.object_patch(store["cases"][ci][1], c, crop, shape, obj_label)
            patch = hn.neg_patch(store["neg"][ci], c, crop, shape)
            trace = {}
            want_pts, want_cnt = hn.clicks(obj, patch, rows[j].astype(np.uint64), params, trace)
            np.testing.assert_array_equal(cnt[j], want_cnt, err_msg=str((samples[j], obj_label)))
            np.testing.assert_array_equal(pts[j], want_pts, err_msg=str((samples[j], obj_label)))
            if not patch.any():
                seen["plain_rows"] += 1
                seen["shallow"] += int(ci == 2)
                continue
            seen["neg_rows"] += 1
            assert cnt[j, 1] <= int(rows[j, 1]) and (cnt[j, 1] > 0) == (rows[j, 1] > 0)
            for z, y, x in pts[j, 1, :cnt[j, 1]]:                                     # EVERY background click is a false positive
                assert patch[z, y, x] == 1
                seen["on_object"] += int(obj[z, y, x])
            seen["stopped"] += int(cnt[j, 1] < rows[j, 1])
            seen["slices"] += int(len(set(pts[j, 1, :cnt[j, 1], 0].tolist())) > 1)
    # case 2 is followed by case 3 in the store, whose first slice holds false positives under the padding slices of a crop
    # (the small crops hold the false positives of one slice at a time)
    assert all(v > 0 for k, v in seen.items() if k != "on_object" and (k != "slices" or shape == LARGE)), seen


def test_clicks_neg_equal_the_reference_records():
    with open(os.path.join(HERE, "golden", "ref_clicks3d_neg.json")) as f:
        fixture = json.load(f)
    groups = {}
    for rec in fixture["records"]:
        groups.setdefault((rec["neg"], rec["depth"], tuple(rec["crop"]), tuple(rec["params"])), []).append(rec)
    for (nname, depth_out, crop, params), recs in groups.items():
        vol, neg = c3.build(hn.NEG_MASKS[nname][0]), hn.build_neg(nname)
        want = fixture["masks"][nname]
        assert c3.checksum(neg) == (want["popcount"], want["index_sum"])
        if nname == "shallow_none":                                                   # the next case of the store holds false
            nxt = hn.rect_volume((2,) + vol.shape[1:], hn.SHALLOW_NEXT)              # positives under the crop's padding slices
            vol, neg = np.concatenate([vol, np.zeros_like(nxt)]), np.concatenate([neg, nxt])
            assert nxt.any() and depth_out == len(vol) and recs[0]["box_via"] == "padded"
        depth = len(c3.VOLUMES[hn.NEG_MASKS[nname][0]][1])
        lb = torch.from_numpy((vol * ref.LB_SCALE).astype(np.uint8)).cuda()
        plane = torch.from_numpy((neg * ref.LB_SCALE).astype(np.uint8)).cuda()
        tab = torch.from_numpy(np.stack([ref.table_row(0, depth, r["centre"], crop) for r in recs])).cuda()
        rows = np.array([r["row"] for r in recs], dtype=np.uint64).astype(np.uint32)
        pts, cnt, status = _run(lb, plane, tab, rows, (depth_out,) + crop, params)
        assert status == 0
        for j, rec in enumerate(recs):
            assert pts[j, 0, :cnt[j, 0]].tolist() == rec["fg"], (rec["id"], rec["row"][2])
            assert pts[j, 1, :cnt[j, 1]].tolist() == rec["bg"], (rec["id"], rec["row"][2])
            assert np.all(pts[j, 0, cnt[j, 0]:] == -1) and np.all(pts[j, 1, cnt[j, 1]:] == -1)


def _abi_call(store, entry, desc, tab, rows, nbytes, fill, plane=None, ws_bytes=None):
    from boxsegliver_amd import _abi
    n = tab.shape[0]
    ctab = guardbuf.guarded_input(torch.from_numpy(rows.view(np.float32)).cuda())
    pts, cnt, status = guardbuf.guarded((n, 2, 4, 3)), guardbuf.guarded((n, 2)), guardbuf.guarded((1,))
    _i32(status).zero_()
    status.snap = status.flat.clone()
    ws = guardbuf.GuardedWorkspace(nbytes)
    ws.fill(fill)
    planes = [_abi.ptr(store["lb"])] + ([_abi.ptr(plane)] if plane is not None else [])
    code = entry(ctypes.byref(desc), *planes, _abi.ptr(tab), ctypes.c_void_p(ctab.ptr()), ctypes.c_void_p(pts.ptr()),
                 ctypes.c_void_p(cnt.ptr()), ctypes.c_void_p(status.ptr()), ctypes.c_void_p(ws.ptr()),
                 nbytes if ws_bytes is None else ws_bytes, _abi.stream_ptr())
    torch.cuda.synchronize()
    assert ctab.check_untouched() and pts.check_untouched() and cnt.check_untouched() and status.check_untouched()
    assert ws.guard_intact()
    return code, pts, cnt, int(_i32(status).item()), ws.buf[ws.off:ws.off + nbytes].clone()


def test_clicks_neg_zero_plane_guard_bands_and_bad_rows(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    samples = _samples(LARGE, 1.4)
    n = len(samples)
    tab = torch.from_numpy(np.stack([ref.table_row(store["base"][ci], ref.DEPTHS[ci], c, crop) for ci, c, crop in samples])).cuda()
    rows = _click_rows(n, 5)
    desc = ops.lits3d_clicks_desc(store["lb"], n, LARGE, 1, REF_CLICKS)
    nbytes = int(lib.unetk_lits3d_clicks_ws_bytes(ctypes.byref(desc)))
    zeros = torch.zeros_like(store["plane"])
    # an all-zero plane: pts, cnt and the whole workspace are the bits of unetk_lits3d_clicks
    for fill in (0x00, 0xFF):
        code_a, pts_a, cnt_a, st_a, ws_a = _abi_call(store, lib.unetk_lits3d_clicks, desc, tab, rows, nbytes, fill)
        code_b, pts_b, cnt_b, st_b, ws_b = _abi_call(store, lib.unetk_lits3d_clicks_neg, desc, tab, rows, nbytes, fill, zeros)
        assert code_a == code_b == 0 and st_a == st_b == 0 and pts_b.unwritten() == 0 and cnt_b.unwritten() == 0
        assert torch.equal(_i32(pts_a), _i32(pts_b)) and torch.equal(_i32(cnt_a), _i32(cnt_b))
        # the workspace is read only where the kernels wrote it: those bytes are equal (a byte neither call wrote keeps the fill)
        assert torch.equal(ws_a, ws_b)
    # the real plane, whatever the workspace held
    want = ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(rows.view(np.int32)).cuda(), LARGE, _status(), 1, REF_CLICKS,
                             neg_slices=store["plane"])
    plain = ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(rows.view(np.int32)).cuda(), LARGE, _status(), 1, REF_CLICKS)
    assert not torch.equal(want[0], plain[0])
    for fill in (0x00, 0xFF):
        code, pts, cnt, status, _ = _abi_call(store, lib.unetk_lits3d_clicks_neg, desc, tab, rows, nbytes, fill, store["plane"])
        assert code == 0 and status == 0 and pts.unwritten() == 0 and cnt.unwritten() == 0
        assert torch.equal(_i32(pts), want[0]) and torch.equal(_i32(cnt), want[1])
    code, pts, cnt, status, _ = _abi_call(store, lib.unetk_lits3d_clicks_neg, desc, tab, rows, nbytes, 0x00, store["plane"], nbytes - 1)
    assert code == -3 and pts.changed_anywhere() == 0 and cnt.changed_anywhere() == 0          # UNETK_E_WORKSPACE, nothing launched
    assert lib.unetk_lits3d_clicks_neg(ctypes.byref(desc), _abi.ptr(store["lb"]), None, _abi.ptr(tab), _abi.ptr(tab), _abi.ptr(tab),
                                       _abi.ptr(tab), _abi.ptr(tab), _abi.ptr(tab), nbytes, _abi.stream_ptr()) == -1
    # rows of draws out of range: bit 2 (value 4), the values clamped, everything in bounds
    bad = rows.copy()
    bad[0, 0], bad[1, 0], bad[2, 1], bad[3, 2], bad[4, 2] = 0, 9, 0xFFFFFFFF, 0, 2
    clamped = bad.copy()
    clamped[0, 0], clamped[1, 0], clamped[2, 1], clamped[3, 2], clamped[4, 2] = 1, 4, 4, 1, 1
    code, pts, cnt, status, _ = _abi_call(store, lib.unetk_lits3d_clicks_neg, desc, tab, bad, nbytes, 0xFF, store["plane"])
    assert code == 0 and status == 4
    ok = ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(clamped.view(np.int32)).cuda(), LARGE, _status(), 1, REF_CLICKS,
                           neg_slices=store["plane"])
    assert torch.equal(_i32(pts), ok[0]) and torch.equal(_i32(cnt), ok[1])
    got = _i32(pts).cpu().numpy()
    assert got.min() >= -1 and got[..., 0].max() < LARGE[0] and got[..., 1].max() < ref.H and got[..., 2].max() < ref.W
    for k in range(5):
        one = rows.copy()
        one[k] = bad[k]
        assert _abi_call(store, lib.unetk_lits3d_clicks_neg, desc, tab, one, nbytes, 0x00, store["plane"])[3] == 4, k
    # hostile sample rows: centres and crops far outside, a case of negative depth, a base outside the store
    wild = tab.clone()
    wild[0, 2:7] = torch.tensor([10 ** 6, -10 ** 6, 10 ** 6, 10 ** 6, -5], dtype=torch.int32)
    wild[1, 0:2] = torch.tensor([10 ** 6, 9], dtype=torch.int32)
    wild[2, 1] = -3
    wild[3, 0] = -10 ** 6
    code, pts, cnt, status, _ = _abi_call(store, lib.unetk_lits3d_clicks_neg, desc, wild, rows, nbytes, 0xFF, store["plane"])
    assert code == 0 and pts.unwritten() == 0 and cnt.unwritten() == 0
    with pytest.raises(AssertionError):
        ops.lits3d_clicks(store["lb"], tab, torch.from_numpy(rows.view(np.int32)).cuda(), LARGE, _status(), 1, REF_CLICKS,
                          neg_slices=store["plane"][:-1])


# ------------------------------------------------------------------------------------------------- end to end
ARGV = ("liver_3d --mode train --tag cli3dhn --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
        "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
        "--num_of_steps 2 --batches_per_epoch 2 --eval_num_batches_per_epoch 2 --eval_per_epoch --evaluator Volume "
        "--primary_metric Tumor/Dice --secondary_metric Liver/Dice --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
        "--learning_rate 0.001 --save_best --log_step 1 --use_spatial").split()
HARD = "--hard_neg_patches 0.25 --hard_neg_clicks".split()


def _write_predictions(directory, cases):
    """predict-<PID>.nii.gz of the two training cases, by hand: the labelled tumour plus false alarms -- a block of 3 x 4 x 5 in
    case 0, one of 2 x 3 x 3 and a speck of 4 voxels (below min_size) in the tumour-free case 1; and a file of a case that
    meta.json does not know, which the tool leaves alone."""
    from boxsegliver_amd.data import nii_kits
    directory.mkdir()
    preds = []
    for pid in (0, 1):
        pred = cases[pid][1].copy()
        if pid == 0:
            pred[8:11, 30:34, 2:7] = 2
            assert not (cases[0][1][7:12, 29:35, 1:8] == 2).any()
        else:
            pred[2:4, 5:8, 30:33] = 2
            pred[6, 20, 20:24] = 2
        preds.append(pred)
        nii_kits.write_nii(pred, None, directory / "predict-{}.nii.gz".format(pid), out_dtype=np.uint8,
                           affine=np.diag([-0.8, -0.8, 2.5, 1.0]))
    nii_kits.write_nii(preds[0], None, directory / "predict-77.nii.gz", out_dtype=np.uint8, affine=np.diag([-0.8, -0.8, 2.5, 1.0]))
    return preds


def test_liver_3d_trains_on_mined_false_positives_from_the_command_line(tmp_path, capsys):
    from boxsegliver_amd.data import extract, lits3d
    from boxsegliver_amd.entry import main as entry
    cases = ref.write_dataset(tmp_path)
    paths = ["--lits_root", str(tmp_path)]
    # 1. a first run
    run0 = tmp_path / "run0"
    assert entry.main(ARGV + paths + ["--model_dir", str(run0)]) == 0
    # 2. its predictions over the training volumes (written by hand), 3. mined by the tool
    preds = _write_predictions(tmp_path / "pred", cases)
    capsys.readouterr()
    extract.main(["neg3d", str(tmp_path / "pred"), str(tmp_path)])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("case 0:") and lines[1].startswith("case 1:")
    neg_dir = tmp_path / "neg3d"
    assert sorted(p.name for p in neg_dir.iterdir()) == ["neg-0.npz", "neg-1.npz"]
    masks = []
    for pid in (0, 1):
        rec = extract.load_neg(neg_dir / "neg-{}.npz".format(pid))
        want_out, want_counts, want_head = hn.fp_mask(preds[pid], cases[pid][1], 2, 2, 6)
        np.testing.assert_array_equal(extract.unpack_neg(rec), want_out)
        assert rec["slice_counts"].tolist() == want_counts.tolist() and (rec["components"], rec["kept"]) == tuple(want_head[:2])
        masks.append(want_out)
    assert masks[0].sum() == 60 and masks[1].sum() == 18
    # 4. the second run's batches
    hard = ARGV + HARD + ["--hard_neg_from", str(neg_dir)] + paths
    args, _, _ = entry.get_arguments(hard + ["--model_dir", str(tmp_path / "run1")])
    params = {"args": args, "lits_root": str(tmp_path)}
    gen = lits3d.input_fn("train", params)
    tstore = params[("lits_store", True)][0]
    np.testing.assert_array_equal(tstore.neg.cpu().numpy(), np.concatenate(masks) * ref.LB_SCALE)
    plain_args, _, _ = entry.get_arguments(ARGV + paths + ["--model_dir", str(tmp_path / "run1")])
    plain_params = {"args": plain_args, "lits_root": str(tmp_path)}
    plain = lits3d.input_fn("train", plain_params)
    differs = 0
    for _ in range(6):
        feats, labels = next(gen)
        pf, pl = next(plain)
        assert feats["images"].shape == (2, 4, 32, 32, 1) and feats["sp_guide"].shape == (2, 4, 32, 32, 2)
        assert bool(torch.isfinite(feats["images"]).all()) and bool(torch.isfinite(feats["sp_guide"]).all())
        differs += int(not torch.equal(feats["sp_guide"], pf["sp_guide"]))
    assert differs > 0
    # eval_online never uses the plane: its batches are those of a run without the flags, bit for bit
    ev, ev_plain = list(lits3d.input_fn("eval_online", params)), list(lits3d.input_fn("eval_online", plain_params))
    assert len(ev) == len(ev_plain) == 2
    for (fa, la), (fb, lb) in zip(ev, ev_plain):
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(fa["sp_guide"], fb["sp_guide"]) and torch.equal(la, lb)
    assert not hasattr(params[("lits_store", False)][0], "neg")
    assert int(params[("lits3d_status", True)].item()) == 0 and int(params[("lits3d_status", False)].item()) == 0
    # the command line: 2 more steps in the first run's directory, from its checkpoint
    assert json.load(open(str(run0 / "checkpoint")))["global_step"] == 2
    assert entry.main(hard + ["--model_dir", str(run0)]) == 0
    assert json.load(open(str(run0 / "checkpoint")))["global_step"] == 4
    losses = [float(v) for v in re.findall(r"loss = ([^,\s]+)", open(str(run0 / "logs" / "train_cli3dhn")).read())]
    assert len(losses) >= 4 and all(np.isfinite(v) for v in losses)
    # a training case without a file: an error naming the case and the path
    (neg_dir / "neg-1.npz").rename(tmp_path / "neg-1.npz")
    with pytest.raises(FileNotFoundError, match=r"case 1 .*neg-1\.npz"):
        lits3d.input_fn("train", {"args": args, "lits_root": str(tmp_path)})
    # slice counts that do not match the mask
    rec = extract.load_neg(neg_dir / "neg-0.npz")
    wrong = rec["slice_counts"].copy()
    wrong[9] += 1
    extract.save_neg(neg_dir / "neg-1.npz", masks[1], masks[1].sum(axis=(1, 2)), 1, 2)
    extract.save_neg(neg_dir / "neg-0.npz", masks[0], wrong, 1, 1)
    with pytest.raises(ValueError, match="slice_counts"):
        lits3d.input_fn("train", {"args": args, "lits_root": str(tmp_path)})


def test_empty_neg_files_give_the_batches_of_a_run_without_the_flag(tmp_path):
    from boxsegliver_amd.data import extract, lits3d
    from boxsegliver_amd.entry import main as entry
    cases = ref.write_dataset(tmp_path)
    neg_dir = tmp_path / "neg3d"
    neg_dir.mkdir()
    for pid in (0, 1):
        empty = np.zeros(cases[pid][1].shape, np.uint8)
        extract.save_neg(neg_dir / "neg-{}.npz".format(pid), empty, empty.sum(axis=(1, 2)), 0, 0)
    paths = ["--lits_root", str(tmp_path), "--model_dir", str(tmp_path / "run")]
    args, _, _ = entry.get_arguments(ARGV + ["--hard_neg_clicks", "--hard_neg_from", str(neg_dir)] + paths)
    plain_args, _, _ = entry.get_arguments(ARGV + paths)
    params = {"args": args, "lits_root": str(tmp_path)}
    gen = lits3d.input_fn("train", params)
    plain = lits3d.input_fn("train", {"args": plain_args, "lits_root": str(tmp_path)})
    assert int(params[("lits_store", True)][0].neg.sum().item()) == 0
    for _ in range(4):
        (fa, la), (fb, lb) = next(gen), next(plain)
        assert torch.equal(fa["images"], fb["images"]) and torch.equal(la, lb)
        assert torch.equal(fa["sp_guide"].view(torch.int32), fb["sp_guide"].view(torch.int32))
    assert int(params[("lits3d_status", True)].item()) == 0
