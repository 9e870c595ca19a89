"""The table of the non-finite tier (tests/nonfinite_cases.py) held honest without a GPU.

For every row and every output: the set R of outputs that must be NaN is not empty and lies inside the set A of outputs that may
be; at least a quarter of the row's main output lies outside A, so the equality half of the device test is never vacuous; and
a float64 restatement of the op on the poisoned inputs is NaN exactly on a set between R and A -- which also holds the clean
reference honest: outside A the restatement of the poisoned inputs equals it bit for bit.  No row is skipped."""
import numpy as np
import pytest

import nonfinite_cases as T


@pytest.mark.parametrize("rid", [r.id for r in T.ROWS])
def test_row_sets_and_restatement(rid):
    row = T.BY_ID[rid]
    c = T.case(row)
    main = T.MAIN[row.fam]
    assert main in c["outs"] and list(c["outs"])[0] == main
    assert all(np.isfinite(v).all() for v in c["inputs"].values() if v is not None), rid
    got = c["restate"](T.poisoned(c))
    for name, (R, A, clean) in c["outs"].items():
        what = "%s %s" % (rid, name)
        assert R.shape == A.shape == clean.shape and R.dtype == bool and A.dtype == bool, what
        assert np.isfinite(clean).all(), what
        assert R.any(), what + ": R is empty"
        assert not (R & ~A).any(), what + ": R is no subset of A"
        nan = np.isnan(np.asarray(got[name], np.float64)).reshape(R.shape)
        assert not (R & ~nan).any(), "%s: the restatement is finite at %d outputs of R" % (what, int((R & ~nan).sum()))
        assert not (nan & ~A).any(), "%s: the restatement is NaN at %d outputs outside A" % (what, int((nan & ~A).sum()))
        assert np.array_equal(np.asarray(got[name], np.float64).reshape(R.shape)[~A], clean[~A]), what + ": moved outside A"
        if name == main:
            share = 1.0 - A.mean()
            assert share >= 0.25, "%s: only %.3f of the outputs lie outside A" % (what, share)
            assert np.any(clean[~A] != 0), what + ": the clean reference is identically zero outside A"


def test_every_family_and_both_halo_kinds_have_rows():
    """Each family of the table is present, filter-tap rows exist whose A is strictly larger than R (the zero halo), and the
    depth-edge rows of the bf16 3-D kernel leave the skipped plane out of R."""
    assert set(T.MAIN) == set(r.fam for r in T.ROWS)
    for fam in ("conv", "aff", "conv1d", "conv3d"):
        halo = [r.id for r in T.rows(fam) if r.operand == "w" and (T.case(r)["outs"][T.MAIN[fam]][1] & ~T.case(r)["outs"][T.MAIN[fam]][0]).any()]
        assert halo, fam
    R, A, _ = T.case(T.BY_ID["c3d_bf16_ft_w_tap0"])["outs"]["y"]
    assert not R[:, 0].any() and A[:, 0, :, :, 7].all() and R[:, 1:, :, :, 7].all()
    R, A, _ = T.case(T.BY_ID["c3d_bf16_ft_w_tap2"])["outs"]["y"]
    assert not R[:, -1].any() and A[:, -1, :, :, 63].all()
    R, A, _ = T.case(T.BY_ID["c3d_live_x"])["outs"]["y"]
    assert not R[..., 120:].any() and A[..., 120:].any() and R[..., :120].any()
    # the subsample rows: of the nine stride-1 positions a poisoned pixel reaches, only the strided ones count
    R, _, _ = T.case(T.BY_ID["c3d_subsample_x_odd"])["outs"]["y"]
    assert R.shape == (1, 2, 4, 6, 32) and int(R[..., 0].sum()) == 1 and R[0, 1, 1, 2].all()
    R, _, _ = T.case(T.BY_ID["c3d_subsample_x_even"])["outs"]["y"]
    assert int(R[..., 0].sum()) == 4 and R[0, 0, 1:3, 2:4].all()
    R, A, _ = T.case(T.BY_ID["c3d_subsample_w_tap22"])["outs"]["y"]
    assert not R[:, :, -1].any() and not R[:, :, :, -1].any() and A[..., 31].all() and R[:, :, :-1, :-1, 31].all()
    # dropped units (mask 0) inside R: NaN * 0 is NaN in the restatement, and so it must be on the device
    for rid in ("fc_x_masked", "fc_w_masked", "fc_b_masked"):
        c = T.case(T.BY_ID[rid])
        assert (c["inputs"]["mask"][c["outs"]["y"][0]] == 0).any() and (c["inputs"]["mask"][c["outs"]["y"][0]] != 0).any(), rid
    # the four places of a pool window, in both storages, for both 2 x 2 pools
    for fam, stem in (("mp2", "mp2_place"), ("normpool", "normpool_place")):
        ids = set(r.id for r in T.rows(fam))
        assert all(stem + "%d%s" % (k, s) in ids for k in range(4) for s in ("", "_bf16s")), fam


def test_payload_patterns_are_nans_and_the_low_one_truncates_to_inf():
    for f32, b16 in T.PAYLOADS:
        assert np.isnan(np.array([f32], np.uint32).view(np.float32)[0])
        assert np.isnan(np.array([b16 << 16], np.uint32).view(np.float32)[0])
    lo = T.PAYLOADS[1][0]
    assert np.isinf(np.array([lo & 0xFFFF0000], np.uint32).view(np.float32)[0])      # what a truncating bf16 store would keep
