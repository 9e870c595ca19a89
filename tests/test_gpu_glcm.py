"""GPU: the `glcm` context guide -- `unetk_glcm_features` (csrc/glcm.hip) against a brute-force count and the numpy
restatement of the reference's property formulas (tests/test_glcm_host.py), its refusals, `data/extract.py
dump_glcm_feature` against the rows recorded from the reference (tests/golden/ref_glcm_feature.npz), the pipeline's rows
under `--glcm --context_list hist 200 glcm 96`, GUNet with a 296-wide context against the oracle, and `main_g liver`
training from files the `glcm` sub-command wrote.

Tolerances.  Counts are exact.  A property is a sum of at most 65,536 fp64 terms; with S_f the sum of the absolute values
of its terms (1 for correlation) the rounding bound of such a sum is 65536 * 2^-53 * S_f ~ 7e-12 * S_f on each side, and the
tests assert |device - reference| <= 1e-9 * S_f (room for the propagated error of the mean and the device's log / sqrt; a
single miscounted pair moves a property by orders of magnitude more).  A patch without pairs gives exactly 0 everywhere
and correlation exactly 1.  A constant patch with pairs has P = 1 on one diagonal entry: contrast, dissimilarity, entropy
(-0.0 == 0), shade and prominence are exactly 0, correlation exactly 1, and homogeneity = energy = 1 exactly (2 after the
level scaling) -- these two are NOT 0, P / (1 + 0) and sqrt(P^2) being 1."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_glcm_host import (OFFSETS, SCALE, fixture, glcm_counts_brute, glcm_counts_numpy, glcm_features_numpy, restated)

pytestmark = pytest.mark.gpu

UNSUPPORTED, BADARG, WORKSPACE = -2, -1, -3


@functools.lru_cache(maxsize=None)
def _batch():
    """The patches of the exact tests and their brute-force counts, made once."""
    rng = np.random.default_rng(42)
    board = np.zeros((4, 6), np.uint8)
    board[::2, 1::2] = 255
    board[1::2, ::2] = 255
    patches = [rng.integers(0, 256, s).astype(np.uint8) for s in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (2, 9))]
    patches += [np.zeros((5, 5), np.uint8), np.full((5, 5), 255, np.uint8), board,
                rng.integers(0, 256, (17, 23)).astype(np.uint8), rng.integers(0, 256, (64, 70)).astype(np.uint8),
                np.full((300, 300), 131, np.uint8)]
    counts = np.stack([glcm_counts_brute(p) for p in patches])
    return tuple(patches), counts


CONSTANT = (6, 7, 11)            # indices of the constant patches in _batch()


@functools.lru_cache(maxsize=None)
def _device(norm_levels=True):
    from boxsegliver_amd import ops
    return ops.glcm_features(list(_batch()[0]), norm_levels=norm_levels, want_counts=True)


def test_counts_equal_the_double_loop():
    patches, ref = _batch()
    sizes = np.cumsum([0] + [p.size for p in patches[:-1]])
    assert (sizes % 2 == 1).sum() >= 5                        # packed back to back: odd byte offsets
    feats, counts = _device()
    assert counts.dtype == np.uint32 and counts.shape == (12, 12, 256, 256) and feats.shape == (12, 96)
    np.testing.assert_array_equal(counts, ref)
    assert counts[11].max() == 2 * 300 * 299 > 65535          # one diagonal entry holds every pair, twice


@pytest.mark.parametrize("n", [1, 37])
def test_counts_of_other_batch_sizes(n):
    from boxsegliver_amd import ops
    rng = np.random.default_rng(n)
    patches = [rng.integers(0, 256, (int(rng.integers(1, 30)), int(rng.integers(1, 30)))).astype(np.uint8) for _ in range(n)]
    if n == 1:
        patches = [_batch()[0][9]]
    feats, counts = ops.glcm_features(patches, want_counts=True)
    np.testing.assert_array_equal(counts, np.stack([glcm_counts_numpy(p) for p in patches]))
    ref = [glcm_features_numpy(p) for p in patches]
    err = np.abs(feats - np.stack([v for v, _ in ref]))
    assert np.all(err <= 1e-9 * np.stack([m for _, m in ref]))


def test_counts_at_the_largest_extent():
    """4096 x 4096, the largest patch the entry point takes (16.7 M pixels through one workgroup, pixel indices up to 2^24),
    with a negative column offset, and the two one-pixel-wide strips of that length; counts by np.bincount."""
    from boxsegliver_amd import ops
    rng = np.random.default_rng(7)
    big = rng.integers(0, 256, (4096, 4096)).astype(np.uint8)
    offsets = [(1, -1), (0, 3)]
    feats, counts = ops.glcm_features([big[0:1].copy(), big, big[:, 5:6].copy()], offsets=offsets, want_counts=True)
    for p, patch in enumerate((big[0:1], big, big[:, 5:6])):
        h, w = patch.shape
        for k, (dr, dc) in enumerate(offsets):
            r0, r1, c0, c1 = max(0, -dr), min(h, h - dr), max(0, -dc), min(w, w - dc)
            ref = np.zeros((256, 256), np.int64)
            if r1 > r0 and c1 > c0:
                a = patch[r0:r1, c0:c1].astype(np.int64).reshape(-1)
                b = patch[r0 + dr:r1 + dr, c0 + dc:c1 + dc].astype(np.int64).reshape(-1)
                ref = np.bincount(a * 256 + b, minlength=65536).reshape(256, 256)
            np.testing.assert_array_equal(counts[p, k], (ref + ref.T).astype(np.uint32))
        ref, mags = glcm_features_numpy(patch, offsets=offsets, counts=counts[p])
        assert np.all(np.abs(feats[p] - ref) <= 1e-9 * mags)
    assert int(counts[1, 0].sum(dtype=np.uint64)) == 2 * 4095 * 4095


def test_properties_match_the_restatement():
    patches, counts = _batch()
    feats, _ = _device()
    assert feats.dtype == np.float64 and np.isfinite(feats).all()
    for p in range(len(patches)):
        ref, mags = glcm_features_numpy(patches[p], counts=counts[p])
        err = np.abs(feats[p] - ref)
        print("patch", patches[p].shape, "max |err| / S_f", float(np.max(err / np.maximum(mags, 1e-300))))
        assert np.all(err <= 1e-9 * mags), (p, err.max())


def test_exact_values_without_pairs_and_on_constant_patches():
    patches, counts = _batch()
    feats = _device()[0].reshape(12, 8, 12)
    pairs = counts.reshape(12, 12, -1).sum(-1) > 0
    assert not pairs[0].any() and (~pairs).sum() > 20 and pairs[CONSTANT, :].all()
    for p in range(12):
        for k in range(12):
            if not pairs[p, k]:
                assert feats[p, 5, k] == 1.0
                assert all(feats[p, f, k] == 0 for f in (0, 1, 2, 3, 4, 6, 7)), (p, k, feats[p, :, k])
    for p in CONSTANT:
        for k in range(12):
            assert feats[p, 5, k] == 1.0
            assert all(feats[p, f, k] == 0 for f in (0, 1, 4, 6, 7)), (p, k, feats[p, :, k])
            assert feats[p, 2, k] == 2.0 and feats[p, 3, k] == 2.0


def test_two_calls_give_the_same_bits_and_the_scaling_is_the_only_difference():
    from boxsegliver_amd import ops
    feats, counts = _device()
    again, counts2 = ops.glcm_features(list(_batch()[0]), want_counts=True)
    assert feats.tobytes() == again.tobytes() and counts.tobytes() == counts2.tobytes()
    raw, _ = _device(False)
    assert (raw.reshape(12, 8, 12) * SCALE[None, :, None]).tobytes() == feats.reshape(12, 8, 12).tobytes()
    only = ops.glcm_features(list(_batch()[0]))                # without the counts: the same features
    assert only.tobytes() == feats.tobytes()


def test_refusals_launch_nothing():
    from guardbuf import GuardedWorkspace
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    V = ctypes.c_void_p
    patch = np.arange(35, dtype=np.uint8).reshape(5, 7)
    pix = torch.from_numpy(np.concatenate([patch.reshape(-1), np.zeros(29, np.uint8)])).cuda()
    tab_buf, off_buf = np.zeros(16, np.int32), np.zeros(80, np.int32)
    tab_buf[:3] = (0, 5, 7)
    off_buf[:24] = np.array(OFFSETS, np.int32).reshape(-1)
    sentinel = 0x7FF8BADBADBADBAD
    out = torch.full((2 * 8 * 16 + 2,), sentinel, dtype=torch.int64, device="cuda")
    counts = torch.full((12 * 65536 + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    nbytes = lib.unetk_glcm_features_ws_bytes(1, 12)
    assert nbytes >= 16
    ws = GuardedWorkspace(nbytes)
    stream = V(torch.cuda.current_stream().cuda_stream)

    def call(table=(0, 5, 7), **kw):
        tab_buf[:3] = table
        a = dict(pix=pix.data_ptr(), pix_bytes=64, tab=tab_buf.ctypes.data, n=1, offs=off_buf.ctypes.data, K=12,
                 out=out.data_ptr(), counts=counts.data_ptr(), ws=ws.ptr(), ws_bytes=nbytes)
        a.update(kw)
        return lib.unetk_glcm_features(V(a["pix"]), a["pix_bytes"], V(a["tab"]), a["n"], V(a["offs"]), a["K"], 1, V(a["out"]),
                                       V(a["counts"]), V(a["ws"]), a["ws_bytes"], stream)

    for n, k in ((0, 12), (-1, 12), (1, 0), (1, 17)):
        assert lib.unetk_glcm_features_ws_bytes(n, k) == 0
        assert call(n=n, K=k) == UNSUPPORTED, (n, k)
    for table in ((0, 0, 7), (0, 4097, 1), (0, 5, 0), (0, 1, 4097), (0, -3, 7)):
        assert call(table) == UNSUPPORTED, table
    assert call(pix_bytes=1 << 31) == UNSUPPORTED
    for name in ("pix", "tab", "offs", "out", "ws"):
        assert call(**{name: None}) == BADARG, name
    shifted = np.zeros(16, np.uint8)                                             # the table 2 bytes off a 4-byte boundary
    shifted[2:14] = np.array((0, 5, 7), np.int32).view(np.uint8)
    assert (shifted.ctypes.data + 2) % 4 == 2
    for kw in (dict(tab=shifted.ctypes.data + 2), dict(offs=off_buf.ctypes.data + 2), dict(out=out.data_ptr() + 4),
               dict(counts=counts.data_ptr() + 2), dict(ws=ws.ptr() + 8)):
        assert call(**kw) == BADARG, kw
    for table in ((30, 5, 7), (64, 1, 1), (-1, 5, 7)):                           # reaches past pix_bytes / starts before it
        assert call(table) == BADARG, table
    assert call(pix_bytes=34) == BADARG
    assert call(ws_bytes=nbytes - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((counts == 0x5A5A5A5A).all()) and ws.guard_intact()
    # and the accepted call: every element of out [1][8][12] and of the counts written, nothing beyond, the workspace guard whole
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:96] != sentinel).all()) and bool((out[96:] == sentinel).all()) and ws.guard_intact()
    assert bool((counts[12 * 65536:] == 0x5A5A5A5A).all())
    got = counts[:12 * 65536].cpu().numpy().view(np.uint32).reshape(12, 256, 256)
    np.testing.assert_array_equal(got, glcm_counts_numpy(patch))
    ref, mags = glcm_features_numpy(patch)
    dev = out[:96].cpu().numpy().view(np.float64).reshape(8, 12).reshape(-1)
    assert np.all(np.abs(dev - ref) <= 1e-9 * mags)


# ----------------------------------------------------------------------------------------------------- the extractor
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_dump_glcm_feature_matches_the_reference_rows(tmp_path, monkeypatch, mode):
    from boxsegliver_amd import ops
    from boxsegliver_amd.data import extract
    cases = fixture()
    nii = tmp_path / "nii"
    nii.mkdir()
    for pid in range(len(cases)):
        (nii / "volume-{}.nii".format(pid)).write_bytes(b"")
    monkeypatch.setattr(extract.nii_kits, "read_lits", lambda pid, obj, path: (None, cases[int(pid)][0 if obj == "vol" else 1]))
    calls = []
    real = ops.glcm_features
    monkeypatch.setattr(ops, "glcm_features", lambda patches, **kw: calls.append(len(patches)) or real(patches, **kw))
    paths = extract.dump_glcm_feature(nii, tmp_path / "feat", mode, [c[2] for c in cases])
    assert [p.name for p in paths] == ["000.npy", "001.npy", "002.npy"] and paths[0].parent == tmp_path / "feat" / "glcm" / mode
    assert len(calls) == 3 and min(calls) >= 6                 # ONE device call per case, with all of its patches
    for pid, (_, _, _, train, ev) in enumerate(cases):
        got, ref = np.load(paths[pid]), (train if mode == "train" else ev)
        assert got.dtype == np.float32 and got.shape == ref.shape
        mags = restated(mode)[pid][1]
        tol = (1e-9 * mags).astype(np.float32).astype(np.float64) + np.spacing(np.maximum(np.abs(got), np.abs(ref))).astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        print("case", pid, mode, "max err / tol", float(np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (pid, float(err.max()))
        assert np.array_equal(got.any(1), ref.any(1))          # the zero rows are the reference's zero rows


# ------------------------------------------------------------------------------------------------------- the pipeline
def _glcm_file_rows(pid, depth, mode_tag):
    rng = np.random.default_rng(100 * pid + int(mode_tag))
    rows = rng.normal(size=(depth, 96)).astype(np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = pid, np.arange(depth), mode_tag, -0.0
    return rows


def _dataset(tmp_path, n_cases=3, depth=6):
    from test_gpu_lits_context import _dataset as hist_dataset
    hist_dataset(tmp_path)
    for mode, tag in (("train", 1.), ("eval", 2.)):
        d = tmp_path / "feat" / "glcm" / mode
        d.mkdir(parents=True)
        for pid in range(n_cases):
            np.save(d / "{:03d}.npy".format(pid), _glcm_file_rows(pid, depth, tag))


def _args(**over):
    from test_gpu_lits_context import _args as context_args
    return context_args(**dict(dict(glcm=True, context_list=["hist", "200", "glcm", "96"]), **over))


def test_train_rows_carry_the_glcm_rows_of_the_label_slice(tmp_path):
    from boxsegliver_amd.data import lits
    _dataset(tmp_path)
    gen = lits.input_fn("train", {"args": _args(), "lits_root": str(tmp_path)})
    for _ in range(4):
        feats, _ = next(gen)
        ctx = feats["context"]
        assert ctx.shape == (8, 296) and ctx.dtype == torch.float32 and ctx.is_cuda
        ctx = ctx.cpu().numpy()
        for j in range(8):
            pid, z = int(ctx[j, 0]), int(ctx[j, 1])             # the hist columns name the sample's case and slice
            assert ctx[j, 200:].tobytes() == _glcm_file_rows(pid, 6, 1.)[z].tobytes()
    # --hist_scale leaves the glcm columns alone
    feats, _ = next(lits.input_fn("train", {"args": _args(hist_scale=4.0), "lits_root": str(tmp_path)}))
    ctx = feats["context"].cpu().numpy()
    assert np.all(ctx[:, 3:200] == np.float32(1.0)) and np.all(ctx[:, 202] == 1.0) and np.all(ctx[:, 200] * 4 == ctx[:, 0])
    feats, _ = next(lits.input_fn("train", {"args": _args(spatial_random=0.0), "lits_root": str(tmp_path)}))
    assert feats["context"].shape == (8, 296) and bool((feats["context"] == 0).all())
    # the gate: the same list without --glcm is refused and names the flag; wrong lengths and re-parameterised features too
    with pytest.raises(ValueError, match="not supported without --glcm"):
        lits.input_fn("train", {"args": _args(glcm=False), "lits_root": str(tmp_path)})
    with pytest.raises(ValueError, match="96"):
        lits.input_fn("train", {"args": _args(context_list=["hist", "200", "glcm", "48"]), "lits_root": str(tmp_path)})
    with pytest.raises(ValueError, match="glcm_distance"):
        lits.input_fn("train", {"args": _args(glcm_distance=[1]), "lits_root": str(tmp_path)})


def test_hist_noise_moves_the_hist_columns_only(tmp_path):
    from boxsegliver_amd.data import lits
    _dataset(tmp_path)
    gen = lits.input_fn("train", {"args": _args(hist_noise=True, glcm_noise=True), "lits_root": str(tmp_path)})
    moved = 0
    for _ in range(5):
        ctx = next(gen)[0]["context"].cpu().numpy()
        for j in range(8):
            pid, z = int(round(float(ctx[j, 0]))), int(round(float(ctx[j, 1])))
            assert ctx[j, 200:].tobytes() == _glcm_file_rows(pid, 6, 1.)[z].tobytes()          # bit-identical, the -0.0 too
        moved += int((ctx[:, 3:200] != np.float32(0.25)).sum())
    assert moved > 5 * 8 * 190


def test_eval_online_serves_the_eval_rows(tmp_path):
    from boxsegliver_amd.data import lits
    _dataset(tmp_path)
    ev = list(lits.input_fn("eval_online", {"args": _args(), "lits_root": str(tmp_path)}))
    assert len(ev) == 3
    for f, _ in ev:
        ctx = f["context"].cpu().numpy()
        assert ctx.shape == (8, 296) and np.all(ctx[:, 2] == 2.0) and np.all(ctx[:, 202] == 2.0)
        assert np.all(ctx[:, 200] == f["names"].numpy()) and np.all(ctx[:, 201] == ctx[:, 1])


# ---------------------------------------------------------------------------------------------------------- the model
def test_gunet_takes_a_296_wide_context():
    """GUNet's context width comes from the tensor: hist 200 + glcm 96 against the oracle, as test_gpu_gunet_combos compares."""
    from test_gpu_gunet import YML, _setup_variant, _whole_net_check, make_args
    yml = dict(YML, context_fc_channels=[32, 16])
    args = make_args(normalizer="instance_norm", use_context=True, side_dropout=0.0, im_height=64, im_width=64)
    model, inputs, net, params, tensors = _setup_variant(args, yml, dict(), ctx_len=296, size=64)
    assert tuple(inputs["context"].shape) == (2, 296) and tuple(inputs["images"].shape[:3]) == (2, 64, 64)
    _whole_net_check(model, inputs, net, params, tensors, args, yml, {"context": tensors[3]})


def test_main_g_trains_from_files_the_glcm_sub_command_wrote(tmp_path):
    """png dataset + hist rows as the context tests make them; NIfTI volumes of the same cases -> `extract glcm` with the
    dataset's meta.json -> `main_g liver --use_context --glcm --context_list hist 200 glcm 96` trains and evaluates."""
    from test_gpu_lits_context import _TRAIN, _dataset as hist_dataset
    from boxsegliver_amd.data import extract, nii_kits
    from boxsegliver_amd.entry import main_g
    hist_dataset(tmp_path)
    nii = tmp_path / "nii"
    nii.mkdir()
    rng = np.random.default_rng(4)
    for pid in range(3):
        vol = rng.normal(60, 60, size=(6, 64, 64)).astype(np.int16)
        nii_kits.write_nii(vol, None, nii / "volume-{}.nii".format(pid), out_dtype=np.int16, affine=np.diag([-0.8, -0.8, 2.5, 1.0]))
    extract.main(["glcm", str(nii), str(tmp_path / "feat"), "--meta", str(tmp_path / "meta.json"), "--mode", "train", "eval"])
    rows = np.load(tmp_path / "feat" / "glcm" / "train" / "001.npy")
    assert rows.shape == (6, 96) and rows.dtype == np.float32
    assert rows[2].any() and rows[3].any() and not rows[[0, 1, 4, 5]].any() and np.isfinite(rows).all()
    assert np.load(tmp_path / "feat" / "glcm" / "eval" / "001.npy").shape == (6, 96)
    run = tmp_path / "run"
    argv = _TRAIN.replace("--context_list hist 200", "--glcm --context_list hist 200 glcm 96").split()
    argv += ["--model_config", "GUNet_DE.yml", "--lits_root", str(tmp_path), "--model_dir", str(run)]
    assert main_g.main(argv) == 0
    assert json.load(open(str(run / "checkpoint")))["global_step"] == 4
    assert os.path.exists(str(run / "checkpoint_best"))
