"""GPU: `unetk_lits_clicks` (csrc/lits_inter.hip) against the click records of tests/golden/ref_clicks.json -- what the
reference's own img_crop, gen_kernel and inter_simulation gave (tests/golden/make_click_fixtures.py) on the label slices of
click_shapes.py, at the smallest shapes where every loop of the three click kernels repeats (DESIGN.md 7.3.5;
test_ref_clicks_host.py asserts that the records hold those situations).  Integers, compared exactly.  Neither the reference
nor its restatement is imported here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import click_shapes as cs
import guardbuf
from lits3d_ref import LB_SCALE, table_row

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_clicks.json")) as _f:
    FIXTURE = json.load(_f)
LAUNCHES = cs.launches()


def _mask(name):
    shape, ellipses, rects = cs.MASKS[name]
    m = cs.build(shape, ellipses, rects)
    want = FIXTURE["masks"][name]
    assert list(m.shape) == want["shape"] and cs.checksum(m) == (want["popcount"], want["index_sum"]), name
    return m


def _records(sid, row):
    recs = [r for r in FIXTURE["records"] if r["id"] == sid and r["row"] == list(row)]
    assert len(recs) == 1, (sid, row)
    return recs[0]


def _inputs(names, recs):
    """(label store uint8 [n, H, W] = label * 64, one single-slice case per mask; sample table; click table) on the device."""
    store = torch.from_numpy(np.stack([_mask(n) * LB_SCALE for n in names]).astype(np.uint8)).cuda()
    tab = np.stack([table_row(si, 1, (0,) + tuple(centre), crop) for _, si, centre, crop, _ in recs])
    ctab = np.array([row for _, _, _, _, row in recs], np.uint32).view(np.int32)
    return store, torch.from_numpy(tab).cuda(), torch.from_numpy(ctab).cuda()


def _want(recs, params):
    pts = np.full((len(recs), 2, 4, 2), -1, np.int32)
    cnt = np.zeros((len(recs), 2), np.int32)
    for j, (sid, _, centre, crop, row) in enumerate(recs):
        r = _records(sid, row)
        assert r["params"] == list(params) and r["centre"] == list(centre) and r["crop"] == list(crop)
        for kind, name in enumerate(("fg", "bg")):
            cnt[j, kind] = len(r[name])
            if r[name]:
                pts[j, kind, :len(r[name])] = r[name]
    return pts, cnt


@pytest.mark.parametrize("launch", LAUNCHES, ids=["{}x{}-{}".format(l[0][0], l[0][1], "_".join(str(v) for v in l[1])) for l in LAUNCHES])
def test_clicks_equal_the_reference_records(launch):
    from boxsegliver_amd import ops
    shape, params, names, recs = launch
    store, tab, ctab = _inputs(names, recs)
    want_p, want_c = _want(recs, params)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    a = ops.lits_clicks(store, tab, ctab, status, 1, params)
    b = ops.lits_clicks(store, tab, ctab, status, 1, params)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                 # two calls, identical bits
    assert int(status.item()) == 0
    pts, cnt = a[0].cpu().numpy(), a[1].cpu().numpy()
    for j, rec in enumerate(recs):
        what = "{} strategy {}".format(rec[0], rec[4][2])
        np.testing.assert_array_equal(cnt[j], want_c[j], err_msg=what)
        np.testing.assert_array_equal(pts[j], want_p[j], err_msg=what)


def test_every_record_is_launched():
    seen = sorted((rec[0], tuple(rec[4])) for launch in LAUNCHES for rec in launch[3])
    assert seen == sorted((r["id"], tuple(r["row"])) for r in FIXTURE["records"]) and len(seen) == 20
    assert sorted(len(launch[3]) for launch in LAUNCHES) == [2, 2, 2, 2, 2, 4, 6]


@pytest.mark.parametrize("sid", [s[0] for s in cs.SHAPES])
def test_one_row_per_shape_inside_guard_bands(sid):
    """The strategy-3 row of every shape alone, its outputs and a workspace of exactly the queried size inside guard bands."""
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    (_, mask, centre, crop, params, rows), = [s for s in cs.SHAPES if s[0] == sid]
    recs = [(sid, 0, centre, crop, rows[1])]
    store, tab, ctab = _inputs([mask], recs)
    want_p, want_c = _want(recs, params)
    desc = ops.lits_inter_desc(store, 1, (1, 1, 1), obj_label=1, clicks=params)
    nbytes = int(lib.unetk_lits_clicks_ws_bytes(ctypes.byref(desc)))
    h, w = cs.MASKS[mask][0]
    assert nbytes == (3 * h * w + 15) // 16 * 16
    pts, cnt, ws = guardbuf.guarded((1, 2, 4, 2)), guardbuf.guarded((1, 2)), guardbuf.GuardedWorkspace(nbytes)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (ctypes.byref(desc), _abi.ptr(store), _abi.ptr(tab), _abi.ptr(ctab), ctypes.c_void_p(pts.ptr()),
            ctypes.c_void_p(cnt.ptr()), _abi.ptr(status), ctypes.c_void_p(ws.ptr()))
    assert lib.unetk_lits_clicks(*args, nbytes, _abi.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert pts.check_untouched() and pts.unwritten() == 0 and cnt.check_untouched() and cnt.unwritten() == 0
    assert ws.guard_intact() and int(status.item()) == 0
    np.testing.assert_array_equal(pts.view.view(torch.int32).cpu().numpy(), want_p)
    np.testing.assert_array_equal(cnt.view.view(torch.int32).cpu().numpy(), want_c)
