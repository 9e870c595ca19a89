"""GPU: `unetk_eval3d_accumulate` (csrc/lits3d.hip) against its float64 restatement (eval3d_ref.py), and
`liver_3d --mode eval --eval_in_patches`: UNet3D scored on whole LiTS cases in sliding windows, from the command line."""
import ctypes
import json

import numpy as np
import pytest
import torch

import eval3d_ref
import guardbuf
import lits3d_ref as ref

pytestmark = pytest.mark.gpu

SMALL = (6, 16, 20)
HW = (ref.H, ref.W)
ZOOMED = (18, 22)                    # int32((16, 20) * 1.125)
FLIPS = [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in range(8)]
ACC_SENTINEL, CNT_SENTINEL = 0x7FBADBAD, -7777


@pytest.fixture(scope="module")
def store():
    host = eval3d_ref.HostStore()
    host.cases = ref.make_cases()
    host.dev_im = torch.from_numpy(host.im.view(np.int16)).cuda()
    host.dev_lb = torch.from_numpy(host.lb).cuda()
    return host


def _rows(store, ci, centres, crop, flips=None):
    flips = FLIPS if flips is None else flips
    return np.stack([ref.table_row(store.offset[ci], ref.DEPTHS[ci], c, crop, flips[j % len(flips)]) for j, c in enumerate(centres)])


def _corners(depth):
    return [(z, y, x) for z in (0, depth - 1) for y in (0, ref.H - 1) for x in (0, ref.W - 1)]


def _case_rows(store, ci, crop):
    """The eight volume corners (one flip combination each), eight overlapping interior rows with all eight flips and a few
    shifted ones; the shallow case 2 gets rows that hang below its depth."""
    depth = ref.DEPTHS[ci]
    mid = (depth // 2, 19, 23)
    centres = _corners(depth) + [mid] * 8 + [(mid[0] - 1, 22, 25), (mid[0] + 1, 12, 30), (depth - 1, 39, 0)]
    return _rows(store, ci, centres, crop)


def _accumulate(store, ci, tab, probs, acc=None, cnt=None, box=None, host_tab=True):
    from boxsegliver_amd import ops
    depth = ref.DEPTHS[ci]
    c = probs.shape[-1]
    if acc is None:
        acc = torch.zeros((depth,) + HW + (c,), dtype=torch.float32, device="cuda")
        cnt = torch.zeros((depth,) + HW, dtype=torch.int32, device="cuda")
    box = eval3d_ref.union_box(tab, SMALL, depth, HW) if box is None else box
    ops.eval3d_accumulate(torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda(), torch.from_numpy(tab).cuda(),
                          SMALL, store.offset[ci], depth, box, acc, cnt, store.dev_im, host_tab=tab if host_tab else None)
    return acc, cnt


# ------------------------------------------------------------------------------------------------- exact placement
@pytest.mark.parametrize("ci", [0, 2])
def test_zoom_one_rows_are_placed_bit_for_bit(store, ci):
    """crop = (H, W): every lerp weight is 0, the probabilities are small integers, so the sums are exact -- acc and cnt
    must equal the restatement bit for bit, and nothing outside the rows' union box may be touched."""
    depth = ref.DEPTHS[ci]
    tab = _case_rows(store, ci, SMALL[1:])
    interior = tab[8:]                                            # a union box smaller than the case
    rng = np.random.default_rng(5 + ci)
    for rows in (tab, interior):
        probs = rng.integers(0, 8, size=(len(rows),) + SMALL + (3,)).astype(np.float32)
        z0, z1, y0, y1, x0, x1 = box = eval3d_ref.union_box(rows, SMALL, depth, HW)
        if rows is interior:
            assert (y1 - y0, x1 - x0) != HW
        else:
            assert box == (0, depth, 0, ref.H, 0, ref.W)
        want_acc = np.full((depth,) + HW + (3,), ACC_SENTINEL, np.int32).view(np.float32)
        want_cnt = np.full((depth,) + HW, CNT_SENTINEL, np.int32)
        want_acc[z0:z1, y0:y1, x0:x1] = 0
        want_cnt[z0:z1, y0:y1, x0:x1] = 0
        acc, cnt = torch.from_numpy(want_acc.copy()).cuda(), torch.from_numpy(want_cnt.copy()).cuda()
        _accumulate(store, ci, rows, probs, acc, cnt, box)
        racc, rcnt = eval3d_ref.accumulate(rows, probs, SMALL, depth, HW)
        assert rcnt.max() >= 8 and (ci != 2 or rcnt.sum() == len(rows) * depth * 16 * 20)   # the shallow case: depth slices per row
        inside = np.zeros((depth,) + HW, bool)
        inside[z0:z1, y0:y1, x0:x1] = True
        want_acc[inside] = racc[inside].astype(np.float32)
        want_cnt[inside] = rcnt[inside]
        assert np.array_equal(racc.astype(np.float32).astype(np.float64), racc)
        np.testing.assert_array_equal(cnt.cpu().numpy(), want_cnt)
        np.testing.assert_array_equal(acc.cpu().numpy().view(np.int32), want_acc.view(np.int32))


# ------------------------------------------------------------------------------------------------- zoomed windows
def test_zoomed_windows_match_the_restatement(store):
    """18 x 22 crops, all flips, C = 3: |acc - ref| <= 2^-24 cnt (16 max|probs| + |ref|) per voxel (eval3d_ref.bound), cnt exact."""
    worst = 0.0
    for ci in (0, 2):
        depth = ref.DEPTHS[ci]
        tab = _case_rows(store, ci, ZOOMED)
        probs = np.random.default_rng(17 + ci).random((len(tab),) + SMALL + (3,), dtype=np.float32)
        acc, cnt = _accumulate(store, ci, tab, probs)
        racc, rcnt = eval3d_ref.accumulate(tab, probs, SMALL, depth, HW)
        np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
        assert rcnt.max() >= 8
        err = np.abs(acc.cpu().numpy().astype(np.float64) - racc)
        bound = eval3d_ref.bound(racc, rcnt, np.abs(probs).max())
        hit = rcnt > 0
        frac = float((err[hit] / bound[hit]).max())
        print("eval3d_accumulate case {}: max error / bound = {:.3f}".format(ci, frac))
        worst = max(worst, frac)
        assert np.all(err <= bound), (ci, frac)
        assert np.all(err[~hit] == 0)
    print("eval3d_accumulate zoomed: worst error / bound = {:.3f}".format(worst))


def test_order_and_reproducibility(store):
    tab = _case_rows(store, 0, ZOOMED)
    probs = np.random.default_rng(23).random((len(tab),) + SMALL + (3,), dtype=np.float32)
    box = eval3d_ref.union_box(tab, SMALL, 12, HW)
    a = _accumulate(store, 0, tab, probs, box=box)
    b = _accumulate(store, 0, tab, probs, box=box)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    k = 7                                                         # one call with [a; b] = a call with a, then one with b
    acc, cnt = _accumulate(store, 0, tab[:k], probs[:k], box=box)
    _accumulate(store, 0, tab[k:], probs[k:], acc, cnt, box=box)
    assert torch.equal(a[0].view(torch.int32), acc.view(torch.int32)) and torch.equal(a[1], cnt)
    # another order gives another rounding somewhere: the row order is part of the result
    perm = np.arange(len(tab))[::-1].copy()
    c = _accumulate(store, 0, tab[perm], probs[perm], box=box)
    assert torch.equal(a[1], c[1]) and not torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------- guard bands, arguments
def test_guard_bands_and_argument_validation(store):
    from boxsegliver_amd import _abi, ops
    lib = _abi.lib()
    ci, depth = 2, ref.DEPTHS[2]                                  # the shallow case: windows hang below the volume
    tab = _case_rows(store, ci, ZOOMED)
    n = len(tab)
    probs = torch.from_numpy(np.random.default_rng(29).random((n,) + SMALL + (3,), dtype=np.float32)).cuda()
    dtab = torch.from_numpy(tab).cuda()
    box = eval3d_ref.union_box(tab, SMALL, depth, HW)
    want = _accumulate(store, ci, tab, probs.cpu().numpy())
    acc = guardbuf.guarded((depth,) + HW + (3,))
    cnt = guardbuf.guarded((depth,) + HW + (1,))                  # int32 counts in a 4-byte guarded buffer
    for g in (acc, cnt):
        g.view.view(torch.int32).zero_()
        g.snap = g.flat.clone()
    gprobs = guardbuf.guarded_input(probs)
    gtab = guardbuf.guarded_input(dtab.view(torch.float32))
    desc = ops.lits3d_desc(store.dev_im, n, SMALL, False)
    cbox = (ctypes.c_int32 * 6)(*box)

    def call(d=desc, t=gtab.ptr(), p=gprobs.ptr(), c=3, base=store.offset[ci], dep=depth, b=cbox, a=acc.ptr(), k=cnt.ptr()):
        return lib.unetk_eval3d_accumulate(ctypes.byref(d), ctypes.c_void_p(t), ctypes.c_void_p(p), c, base, dep, b,
                                           ctypes.c_void_p(a), ctypes.c_void_p(k), _abi.stream_ptr())
    # rejected inputs launch nothing
    big = ops.lits3d_desc(store.dev_im, n, (2048, 1024, 1024), False)
    assert call(d=big) == -2                                                          # UNETK_E_UNSUPPORTED, as unetk_lits_patch3d
    assert call(p=None) == -1 and call(t=None) == -1 and call(a=None) == -1 and call(k=None) == -1 and call(b=None) == -1
    assert call(c=0) == -1 and call(c=9) == -1
    for bad in ((0, depth + 1, 0, 40, 0, 48), (-1, depth, 0, 40, 0, 48), (0, depth, 0, 41, 0, 48), (0, depth, 0, 40, 0, 49),
                (0, depth, 5, 5, 0, 48), (0, depth, 0, 40, 9, 3)):
        assert call(b=(ctypes.c_int32 * 6)(*bad)) == -1, bad
    assert call(dep=0) == -1 and call(base=-1) == -1 and call(base=store.im.shape[0]) == -1   # a case outside the store
    torch.cuda.synchronize()
    assert acc.changed_anywhere() == 0 and cnt.changed_anywhere() == 0
    # a row of another case contributes nothing on the device; the wrapper, which has the host table, refuses it
    assert call(base=store.offset[3], dep=depth) == 0 and call(dep=depth - 1, b=(ctypes.c_int32 * 6)(0, depth - 1, 0, 40, 0, 48)) == 0
    torch.cuda.synchronize()
    assert acc.changed_anywhere() == 0 and cnt.changed_anywhere() == 0
    foreign = tab.copy()
    foreign[3, 0] = store.offset[3]
    with pytest.raises(_abi.UnetkError, match="base, depth"):
        _accumulate(store, ci, foreign, probs.cpu().numpy())
    foreign = tab.copy()
    foreign[5, 1] = depth + 1
    with pytest.raises(_abi.UnetkError, match="base, depth"):
        _accumulate(store, ci, foreign, probs.cpu().numpy())
    with pytest.raises(_abi.UnetkError, match="device tensors"):
        ops.eval3d_accumulate(probs.cpu(), dtab.cpu(), SMALL, store.offset[ci], depth, box, want[0].cpu(), want[1].cpu(),
                              store.dev_im.cpu())
    # the call itself, inside guard bands
    assert call() == 0
    torch.cuda.synchronize()
    assert acc.check_untouched() and cnt.check_untouched() and gprobs.check_untouched() and gtab.check_untouched()
    assert gprobs.changed_anywhere() == 0 and gtab.changed_anywhere() == 0
    assert torch.equal(acc.view.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(cnt.view.view(torch.int32)[..., 0], want[1])


# ------------------------------------------------------------------------------------------------- round trip
def test_round_trip_with_the_patch_kernel(store):
    """Windows of the plan cut over case 0 by unetk_lits_patch3d, probs = one-hot of the window's labels scaled to
    {0.75, 0.125, 0.125} (dyadic), accumulated and argmaxed: equal to the same pipeline in the restatement at EVERY
    voxel -- the restatement's top-two gap is asserted to exceed the bound everywhere, so no voxel is left out."""
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import lits3d
    ci, depth = 0, ref.DEPTHS[0]
    im, lb = store.cases[ci]
    tables = list(lits3d.eval_tables(store.meta[ci], store, SMALL, 0.5, FLIPS, 32))
    acc = torch.zeros((depth,) + HW + (3,), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((depth,) + HW, dtype=torch.int32, device="cuda")
    racc = rcnt = None
    for tab in tables:
        dtab = torch.from_numpy(tab).cuda()
        _, labels = ops.lits_patch3d(store.dev_im, store.dev_lb, dtab, SMALL, False, 2)
        want_lab = np.stack([ref.patch(im, lb, r[2:5], r[5:7], SMALL, tuple(r[7:10]))[1] for r in tab])
        np.testing.assert_array_equal(labels.cpu().numpy(), want_lab)
        probs = torch.full(labels.shape + (3,), 0.125, dtype=torch.float32, device="cuda")
        probs.scatter_(-1, labels.long().unsqueeze(-1), 0.75)
        ops.eval3d_accumulate(probs, dtab, SMALL, store.offset[ci], depth, lits3d.table_box(tab, SMALL, depth, HW), acc, cnt,
                              store.dev_im, host_tab=tab)
        rprobs = np.full(want_lab.shape + (3,), 0.125)
        np.put_along_axis(rprobs, want_lab[..., None], 0.75, axis=-1)
        racc, rcnt = eval3d_ref.accumulate(tab, rprobs, SMALL, depth, HW, racc, rcnt)
    assert len(tables) == 12 and rcnt.min() >= 8
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    gap = eval3d_ref.top_two_gap(racc)
    bound = eval3d_ref.bound(racc, rcnt, 0.75).max(axis=-1)
    print("round trip: smallest top-two gap / bound = {:.1f}".format(float((gap / bound).min())))
    assert np.all(gap > 2 * bound)                                # either value may move by the bound
    amax, _ = ops.head_predict(acc.view(-1, 3), 3, want_preds=False)
    got = amax.view(cnt.shape).cpu().numpy()
    np.testing.assert_array_equal(got, np.argmax(racc, axis=-1))
    assert {int(v) for v in np.unique(got)} == {0, 1, 2}
    assert (got == lb).mean() > 0.97                               # and it is the case's own label volume, up to two resizes


# ------------------------------------------------------------------------------------------------- end to end
def test_liver_3d_evaluates_whole_cases_in_windows(tmp_path, monkeypatch):
    from boxsegliver_amd import ops
    from boxsegliver_amd.entry import main as entry
    ref.write_dataset(tmp_path)
    run = tmp_path / "run"
    argv = ("liver_3d --mode train --tag cli3d --model UNet3D --classes Liver Tumor --test_fold 1 --im_depth 4 --im_height 32 "
            "--im_width 32 --im_channel 1 --random_flip 7 --tumor_percent 0.5 --batch_size 2 --normalizer instance_norm "
            "--num_of_steps 4 --batches_per_epoch 2 --evaluator Volume --loss_weight_type numerical --loss_numeric_w 0.2 0.4 4.4 "
            "--learning_rate 0.001 --log_step 1").split()
    argv += ["--lits_root", str(tmp_path), "--model_dir", str(run)]
    assert entry.main(argv) == 0
    ev = list(argv)
    ev[ev.index("--mode") + 1] = "eval"
    ev[ev.index("--batch_size") + 1] = "8"
    ev += "--eval_in_patches --eval_mirror --eval_final --save_predict".split()
    assert entry.main(ev) == 0
    results = json.load(open(str(run / "prediction" / "results.json")))
    for key in ("Liver/Dice", "Tumor/Dice", "GLiverDice", "GTumorDice"):
        assert np.isfinite(results[key]) and 0.0 <= results[key] <= 1.0, (key, results)

    # once more, recording what the accumulate step is fed, and the class volumes that are scored
    records, volumes = [], []
    real_acc, real_predict = ops.eval3d_accumulate, ops.head_predict

    def recording_acc(probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=None):
        records.append((sample_tab.cpu().numpy(), probs.cpu().numpy(), int(case_base), int(case_depth), tuple(box)))
        return real_acc(probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=host_tab)

    def recording_predict(probs, ncls, want_preds=True):
        out = real_predict(probs, ncls, want_preds)
        if not want_preds:
            volumes.append(out[0].cpu().numpy())
        return out
    monkeypatch.setattr(ops, "eval3d_accumulate", recording_acc)
    monkeypatch.setattr(ops, "head_predict", recording_predict)
    args, sub, pipe = entry.get_arguments(ev)
    again = entry.run(args, sub, pipe)
    monkeypatch.undo()
    assert again == results
    shape = (4, 32, 32)
    per_case = {}
    for tab, probs, base, depth, box in records:
        assert len(tab) <= 8 and (tab[:, 0] == base).all() and (tab[:, 1] == depth).all()      # a batch never mixes cases
        assert box == eval3d_ref.union_box(tab, shape, depth, HW)
        per_case.setdefault((base, depth), []).append((tab, probs))
    assert sorted(per_case) == [(0, ref.DEPTHS[2]), (ref.DEPTHS[2], ref.DEPTHS[3])] and len(volumes) == 2
    total = excluded = 0
    for (base, depth), got in zip(sorted(per_case), volumes):
        racc = rcnt = None
        max_prob = 0.0
        rows = 0
        for tab, probs in per_case[(base, depth)]:
            racc, rcnt = eval3d_ref.accumulate(tab, probs, shape, depth, HW, racc, rcnt)
            max_prob = max(max_prob, float(np.abs(probs).max()))
            rows += len(tab)
            assert set(map(tuple, tab[:, 7:10])) == set(FLIPS)
        assert rows % 8 == 0 and rcnt.min() >= 8 and len(set(np.unique(rcnt) % 8)) == 1          # uniform over the variants
        sure = eval3d_ref.top_two_gap(racc) > eval3d_ref.bound(racc, rcnt, max_prob).max(axis=-1)
        want = np.argmax(racc, axis=-1)
        got = got.reshape(want.shape)
        np.testing.assert_array_equal(got[sure], want[sure])
        total += sure.size
        excluded += int((~sure).sum())
    print("liver_3d eval: {} of {} voxels excluded (top-two gap within the rounding bound)".format(excluded, total))
    assert excluded <= 0.01 * total
    # the other way of the reference, one forward over the case, stays unbuilt
    plain = [a for a in ev if a != "--eval_in_patches"]
    with pytest.raises(NotImplementedError, match="whole-volume 3-D evaluation"):
        entry.main(plain)
