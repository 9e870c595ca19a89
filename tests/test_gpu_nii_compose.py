"""GPU: `unetk_nii_compose` (ops.nii_compose) -- the post-processed masks of a case composed into the whole volume in NIfTI
file order -- must be BIT-equal to the host path the repository already pins:
nii_kits.write_nii(np.pad(liver + tumor, pad_with), header, path, special=...) read back raw with nii_kits.load.

Every value is a small integer (0, 1 or 2), so there is no tolerance to speak of.  Shapes: a (5, 6, 7) case for all 6
permutations x 8 flip sets x special with every kind of box; (3, 33, 70) and (2, 65, 34) put rows that are no multiple of
the 8-element store group and planes that are no multiple of the 64 x 64 transpose tile (more than one tile along both
axes, with a ragged edge) through the coalesced, x-flipped and transposed paths."""
import itertools

import numpy as np
import pytest
import torch

import guardbuf
from boxsegliver_amd.data import nii_kits

pytestmark = pytest.mark.gpu


def _affine(perm, signs):
    aff = np.zeros((3, 4))
    for i in range(3):
        aff[i, perm[i]] = signs[i] * (0.75 + 0.5 * i)
    return aff


def _header(aff, case):
    trans_bk, _ = nii_kits.file_orientation(nii_kits.Nifti1Header((1, 1, 1), np.int16, sform=aff))
    return nii_kits.Nifti1Header(tuple(case[a] for a in trans_bk), np.int16, (1.0, 1.0, 1.0), sform=aff)


def _oracle(tmp_path, liver, tumor, origin, case, header, special):
    """The file's int16 data, flat with file axis 0 fastest, by write_nii + load."""
    total = np.zeros(liver.shape if liver is not None else tumor.shape, np.uint8)
    for m in (liver, tumor):
        if m is not None:
            total = total + m
    pad_with = tuple((o, n - o - b) for o, b, n in zip(origin, total.shape, case))
    path = tmp_path / "oracle.nii"
    nii_kits.write_nii(np.pad(total, pad_with, mode="constant", constant_values=0), header, path, special=special)
    _, data = nii_kits.load(path)
    assert data.shape == header.shape
    return data.astype(np.int16).reshape(-1, order="F")


def _masks(rng, box):
    """Random masks; tumor voxels both inside the liver and outside it."""
    liver = (rng.rand(*box) < 0.6).astype(np.uint8)
    tumor = (rng.rand(*box) < 0.3).astype(np.uint8)
    return liver, tumor


def _compose(ops, liver, tumor, origin, case, header, special, out=None):
    trans_bk, flips = nii_kits.file_orientation(header, special)
    dev = [None if m is None else torch.from_numpy(m).cuda() for m in (liver, tumor)]
    return ops.nii_compose(dev[0], dev[1], origin, case, trans_bk, flips, out=out)


CASE = (5, 6, 7)
BOXES = [((2, 3, 3), (1, 1, 2)),                                           # interior
         ((2, 3, 3), (0, 1, 2)), ((2, 3, 3), (1, 0, 2)), ((2, 3, 3), (1, 1, 0)),      # touching each low face
         ((2, 3, 3), (3, 1, 2)), ((2, 3, 3), (1, 3, 2)), ((2, 3, 3), (1, 1, 4)),      # touching each high face
         (CASE, (0, 0, 0)),                                                # the whole case
         ((1, 1, 1), (4, 2, 3))]                                           # a single voxel


def test_every_orientation_box_and_pointer_set(tmp_path):
    from boxsegliver_amd import ops
    rng = np.random.RandomState(0)
    n = 0
    combos = list(itertools.product(itertools.permutations(range(3)), itertools.product((1.0, -1.0), repeat=3), (False, True)))
    assert len(combos) == 96
    for k, (perm, signs, special) in enumerate(combos):
        header = _header(_affine(perm, signs), CASE)
        # every box with every orientation would be 96 x 9 x 3 round trips through a file; each orientation takes three
        # boxes and the pointer sets in turn, so that every (box, pointer set) pair meets each of the 6 permutations and both
        # directions of every axis many times over
        for j in range(3):
            box, origin = BOXES[(k + 3 * j) % len(BOXES)]
            liver, tumor = _masks(rng, box)
            which = (k + j) % 3
            liver, tumor = (liver, tumor) if which == 0 else ((liver, None) if which == 1 else (None, tumor))
            ref = _oracle(tmp_path, liver, tumor, origin, CASE, header, special)
            got = _compose(ops, liver, tumor, origin, CASE, header, special)
            assert got.dtype == torch.int16 and got.shape == (5 * 6 * 7,)
            np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=str((perm, signs, special, box, origin, which)))
            n += 1
    assert n == 288


@pytest.mark.parametrize("case,box,origin", [((3, 33, 70), (2, 20, 41), (1, 9, 17)), ((2, 65, 34), (2, 65, 34), (0, 0, 0)),
                                             ((2, 65, 34), (1, 64, 9), (1, 1, 25)), ((3, 33, 70), (3, 1, 70), (0, 32, 0))])
@pytest.mark.parametrize("perm,signs", [((0, 1, 2), (-1.0, -1.0, 1.0)),      # identity: LiTS's own orientation
                                        ((0, 1, 2), (1.0, -1.0, 1.0)),       # x flipped
                                        ((0, 1, 2), (1.0, 1.0, -1.0)),       # x, y and z flipped
                                        ((1, 0, 2), (-1.0, -1.0, 1.0)),      # file axis 0 along y, x along file axis 1
                                        ((2, 0, 1), (1.0, -1.0, -1.0)),      # file axis 0 along y, x along file axis 2, flips
                                        ((2, 1, 0), (-1.0, 1.0, 1.0))])      # file axis 0 along z
def test_tile_and_vector_edges(tmp_path, case, box, origin, perm, signs):
    from boxsegliver_amd import ops
    rng = np.random.RandomState(1)
    header = _header(_affine(perm, signs), case)
    liver, tumor = _masks(rng, box)
    for special in (False, True):
        ref = _oracle(tmp_path, liver, tumor, origin, case, header, special)
        got = _compose(ops, liver, tumor, origin, case, header, special)
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    # a destination offset by one element: not 16-byte aligned, the one-element kernel (coalesced orientations)
    n = case[0] * case[1] * case[2]
    buf = torch.full((n + 9,), -7, dtype=torch.int16, device="cuda")
    got = _compose(ops, liver, tumor, origin, case, header, True, out=buf[1:n + 1])
    assert got.data_ptr() == buf.data_ptr() + 2 and got.data_ptr() % 16 != 0
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    assert int(buf[0]) == -7 and bool((buf[n + 1:] == -7).all())


def _guarded_bytes(mask):
    """A uint8 mask inside a poisoned guardbuf allocation: its bytes travel as 16-bit elements (one pad byte when odd), and
    the poison's bytes (0x49, 0x71) would show up in a sum as values no mask holds."""
    flat = torch.from_numpy(mask).reshape(-1)
    if flat.numel() % 2:
        flat = torch.cat([flat, torch.zeros(1, dtype=torch.uint8)])
    return guardbuf.guarded_input(flat.cuda().view(torch.bfloat16))


@pytest.mark.parametrize("perm,signs,offset", [((0, 1, 2), (-1.0, -1.0, 1.0), 0), ((0, 1, 2), (1.0, 1.0, -1.0), 0),
                                               ((0, 1, 2), (1.0, -1.0, 1.0), 1), ((1, 0, 2), (1.0, -1.0, 1.0), 0),
                                               ((2, 1, 0), (-1.0, 1.0, -1.0), 1)])
def test_guard_bands(tmp_path, perm, signs, offset):
    """Nothing outside the output view changes, no sentinel is left inside it, and the inputs' allocations are untouched."""
    from boxsegliver_amd import _abi
    rng = np.random.RandomState(2)
    case, box, origin = (3, 33, 70), (2, 21, 43), (1, 12, 27)
    header = _header(_affine(perm, signs), case)
    liver, tumor = _masks(rng, box)
    ref = _oracle(tmp_path, liver, tumor, origin, case, header, False)
    n = ref.size
    out = guardbuf.guarded((n + 8,), torch.bfloat16)                # the view: n elements from `offset` on
    view = out.view[offset:offset + n]
    out.mask[:] = False
    out.mask[out.guard + offset:out.guard + offset + n] = True
    g_liver, g_tumor = _guarded_bytes(liver), _guarded_bytes(tumor)
    trans_bk, flips = nii_kits.file_orientation(header, False)
    code = _abi.lib().unetk_nii_compose(
        g_liver.ptr(), g_tumor.ptr(), box[0], box[1], box[2], origin[0], origin[1], origin[2], case[0], case[1], case[2],
        trans_bk[0], trans_bk[1], trans_bk[2], int(flips[0]) | int(flips[1]) << 1 | int(flips[2]) << 2, view.data_ptr(),
        _abi.stream_ptr())
    assert code == 0
    torch.cuda.synchronize()
    assert out.check_untouched() and out.unwritten() == 0
    assert g_liver.changed_anywhere() == 0 and g_tumor.changed_anywhere() == 0
    np.testing.assert_array_equal(view.view(torch.int16).cpu().numpy(), ref)
