"""NIfTI-1 volumes of the LiTS dataset -- host-side mirror of the reference's DataLoader/Liver/nii_kits.py:21-75
(`read_lits`, `read_nii`, `write_nii`) without nibabel (not installed here): a minimal single-file NIfTI-1 codec
(.nii / .nii.gz, 348-byte header, the scalar datatypes LiTS uses) plus the reference's orientation rule.

Orientation (nii_kits.py:33-50): with A = best affine (sform if sform_code > 0, else qform if qform_code > 0, else the
pixdim scaling -- nibabel's `get_best_affine`), `trans[i]` = the data axis world axis i runs along; the array is
transposed to (z, y, x) and flipped so that x decreases, y decreases and z increases with the index; LiTS cases
28..47 (volumes) / 28..51 (labels) are additionally flipped in x ("special").
"""
import gzip
import struct

import numpy as np

_DTYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16,
           768: np.uint32}
_CODES = {np.dtype(v): k for k, v in _DTYPES.items()}


class Nifti1Header(object):
    """The header fields the pipeline uses."""

    def __init__(self, shape, dtype, pixdim=(1.0, 1.0, 1.0), sform=None, qform_code=0, quatern=(0.0, 0.0, 0.0),
                 qoffset=(0.0, 0.0, 0.0), qfac=1.0, scl_slope=0.0, scl_inter=0.0, vox_offset=352.0, endian="<"):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.pixdim = tuple(float(p) for p in pixdim)
        self.sform = None if sform is None else np.asarray(sform, np.float64).reshape(3, 4)
        self.qform_code = int(qform_code)
        self.quatern, self.qoffset, self.qfac = tuple(quatern), tuple(qoffset), float(qfac)
        self.scl_slope, self.scl_inter = float(scl_slope), float(scl_inter)
        self.vox_offset = float(vox_offset)
        self.endian = endian

    def get_zooms(self):
        return self.pixdim[:len(self.shape)]

    def get_data_shape(self):
        return self.shape

    def get_qform(self):
        b, c, d = self.quatern
        a2 = 1.0 - (b * b + c * c + d * d)
        a = np.sqrt(a2) if a2 > 0 else 0.0
        rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                        [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                        [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
        zooms = np.array(self.pixdim[:3], np.float64).copy()
        zooms[2] *= -1.0 if self.qfac < 0 else 1.0
        aff = np.eye(4)
        aff[:3, :3] = rot * zooms[None, :]
        aff[:3, 3] = self.qoffset
        return aff

    def get_best_affine(self):
        """nibabel's rule: sform, else qform, else the pixdim scaling (centre shift omitted: only the axes are used)."""
        if self.sform is not None:
            aff = np.eye(4)
            aff[:3, :] = self.sform
            return aff
        if self.qform_code > 0:
            return self.get_qform()
        aff = np.eye(4)
        aff[0, 0], aff[1, 1], aff[2, 2] = self.pixdim[:3]
        aff[0, 0] *= -1.0          # nibabel's base affine is LAS+ -> RAS flips x
        return aff


def _open(path, mode):
    path = str(path)
    return gzip.open(path, mode) if path.endswith(".gz") else open(path, mode)


def load(file_name):
    """-> (Nifti1Header, raw array in file order [x, y, z], scaling applied as float64 like nibabel's get_fdata)."""
    with _open(file_name, "rb") as f:
        raw = f.read()
    endian = "<"
    if struct.unpack("<i", raw[:4])[0] != 348:
        endian = ">"
        if struct.unpack(">i", raw[:4])[0] != 348:
            raise ValueError("{}: not a NIfTI-1 file (sizeof_hdr != 348)".format(file_name))
    if raw[344:348] not in (b"n+1\0", b"ni1\0"):
        raise ValueError("{}: bad NIfTI-1 magic {!r}".format(file_name, raw[344:348]))
    if raw[344:348] == b"ni1\0":
        raise ValueError("{}: header/image pairs (.hdr/.img) are not supported".format(file_name))
    dim = struct.unpack(endian + "8h", raw[40:56])
    ndim = dim[0]
    if not 1 <= ndim <= 7:
        raise ValueError("{}: bad dim[0] = {}".format(file_name, ndim))
    shape = tuple(d for d in dim[1:1 + ndim])
    while len(shape) > 3 and shape[-1] == 1:
        shape = shape[:-1]
    datatype, = struct.unpack(endian + "h", raw[70:72])
    if datatype not in _DTYPES:
        raise ValueError("{}: unsupported NIfTI datatype {}".format(file_name, datatype))
    pixdim = struct.unpack(endian + "8f", raw[76:108])
    vox_offset, scl_slope, scl_inter = struct.unpack(endian + "3f", raw[108:120])
    qform_code, sform_code = struct.unpack(endian + "2h", raw[252:256])
    quatern = struct.unpack(endian + "3f", raw[256:268])
    qoffset = struct.unpack(endian + "3f", raw[268:280])
    srow = struct.unpack(endian + "12f", raw[280:328])
    hdr = Nifti1Header(shape, _DTYPES[datatype], pixdim[1:4], srow if sform_code > 0 else None, qform_code, quatern,
                       qoffset, -1.0 if pixdim[0] < 0 else 1.0, scl_slope, scl_inter, vox_offset, endian)
    count = int(np.prod(shape))
    dt = np.dtype(_DTYPES[datatype]).newbyteorder(endian)
    data = np.frombuffer(raw, dt, count, int(vox_offset)).reshape(shape, order="F")
    data = data.astype(np.float64)
    if scl_slope not in (0.0,) and not np.isnan(scl_slope):
        data = data * scl_slope + scl_inter
    return hdr, data


def save(data_xyz, header, out_path):
    """Write `data_xyz` (file order [x, y, z]) with `header`'s geometry (dtype from the array)."""
    data_xyz = np.asarray(data_xyz)
    dt = np.dtype(data_xyz.dtype)
    if dt not in _CODES:
        raise ValueError("unsupported dtype {}".format(dt))
    h = bytearray(352)
    struct.pack_into("<i", h, 0, 348)
    dims = [data_xyz.ndim] + list(data_xyz.shape) + [1] * (7 - data_xyz.ndim)
    struct.pack_into("<8h", h, 40, *dims)
    struct.pack_into("<h", h, 70, _CODES[dt])
    struct.pack_into("<h", h, 72, dt.itemsize * 8)
    pix = [header.qfac] + list(header.pixdim[:3]) + [1.0] * 4
    struct.pack_into("<8f", h, 76, *pix)
    struct.pack_into("<3f", h, 108, 352.0, header.scl_slope, header.scl_inter)
    struct.pack_into("<2h", h, 252, header.qform_code, 1 if header.sform is not None else 0)
    struct.pack_into("<3f", h, 256, *header.quatern)
    struct.pack_into("<3f", h, 268, *header.qoffset)
    if header.sform is not None:
        struct.pack_into("<12f", h, 280, *np.asarray(header.sform, np.float32).reshape(-1))
    h[344:348] = b"n+1\0"
    with _open(out_path, "wb") as f:
        f.write(bytes(h))
        f.write(np.asfortranarray(data_xyz).astype(dt.newbyteorder("<")).tobytes(order="F"))


def _orient(affine):
    trans = np.argmax(np.abs(affine[:3, :3]), axis=1)
    return trans, (affine[0, trans[0]] > 0, affine[1, trans[1]] > 0, affine[2, trans[2]] < 0)


def read_nii(file_name, out_dtype=np.int16, special=False, only_header=False):
    """nii_kits.py:33-50: -> (header, data [z, y, x])."""
    vh, data = load(file_name)
    if only_header:
        return vh
    trans, (flip_x, flip_y, flip_z) = _orient(vh.get_best_affine())
    data = data.astype(out_dtype).transpose(*trans[::-1])
    if special:
        data = np.flip(data, axis=2)
    if flip_x:                                  # Increase x from Right to Left
        data = np.flip(data, axis=2)
    if flip_y:                                  # Increase y from Anterior to Posterior
        data = np.flip(data, axis=1)
    if flip_z:                                  # Increase z from Interior to Superior
        data = np.flip(data, axis=0)
    return vh, data


def read_lits(num, obj, file_name, only_header=False):
    """nii_kits.py:21-30: the x-flipped LiTS cases."""
    if obj == "vol":
        return read_nii(file_name, out_dtype=np.int16, special=28 <= int(num) < 48, only_header=only_header)
    if obj == "lab":
        return read_nii(file_name, out_dtype=np.uint8, special=28 <= int(num) < 52, only_header=only_header)
    raise ValueError("obj must be 'vol' or 'lab'")


def write_nii(data, header, out_path, out_dtype=np.int16, special=False, affine=None):
    """nii_kits.py:53-75: the inverse of read_nii (data [z, y, x] -> file order)."""
    if header is not None:
        affine = header.get_best_affine()
    affine = np.asarray(affine, np.float64)
    assert len(np.where(affine[:3, :3].reshape(-1) != 0)[0]) == 3, affine
    trans, (flip_x, flip_y, flip_z) = _orient(affine)
    trans_bk = [int(np.argwhere(np.array(trans[::-1]) == i)[0][0]) for i in range(3)]
    if special:
        data = np.flip(data, axis=2)
    if flip_x:
        data = np.flip(data, axis=2)
    if flip_y:
        data = np.flip(data, axis=1)
    if flip_z:
        data = np.flip(data, axis=0)
    out_image = np.transpose(data, trans_bk).astype(out_dtype)
    if header is None:
        zooms = np.abs(affine[:3, :3]).max(axis=0)
        header = Nifti1Header(out_image.shape, out_dtype, zooms, sform=affine[:3, :])
    save(out_image, header, out_path)


# ----------------------------------------------------------------------------- saved predictions (--save_predict)
SAVE_GZIP_LEVEL = 1         # nibabel's default; mtime 0 and no stored file name make two runs write identical bytes


def _parse_header(raw, file_name):
    """The fields of `load` from a file's first 352 bytes."""
    if len(raw) < 348:
        raise ValueError("{}: shorter than a NIfTI-1 header".format(file_name))
    endian = "<"
    if struct.unpack("<i", raw[:4])[0] != 348:
        endian = ">"
        if struct.unpack(">i", raw[:4])[0] != 348:
            raise ValueError("{}: not a NIfTI-1 file (sizeof_hdr != 348)".format(file_name))
    if raw[344:348] != b"n+1\0":
        raise ValueError("{}: bad or unsupported NIfTI-1 magic {!r}".format(file_name, raw[344:348]))
    dim = struct.unpack(endian + "8h", raw[40:56])
    ndim = dim[0]
    if not 1 <= ndim <= 7:
        raise ValueError("{}: bad dim[0] = {}".format(file_name, ndim))
    shape = tuple(d for d in dim[1:1 + ndim])
    while len(shape) > 3 and shape[-1] == 1:
        shape = shape[:-1]
    datatype, = struct.unpack(endian + "h", raw[70:72])
    if datatype not in _DTYPES:
        raise ValueError("{}: unsupported NIfTI datatype {}".format(file_name, datatype))
    pixdim = struct.unpack(endian + "8f", raw[76:108])
    vox_offset, scl_slope, scl_inter = struct.unpack(endian + "3f", raw[108:120])
    qform_code, sform_code = struct.unpack(endian + "2h", raw[252:256])
    quatern = struct.unpack(endian + "3f", raw[256:268])
    qoffset = struct.unpack(endian + "3f", raw[268:280])
    srow = struct.unpack(endian + "12f", raw[280:328])
    return Nifti1Header(shape, _DTYPES[datatype], pixdim[1:4], srow if sform_code > 0 else None, qform_code, quatern,
                        qoffset, -1.0 if pixdim[0] < 0 else 1.0, scl_slope, scl_inter, vox_offset, endian)


def load_header(file_name):
    """The header alone: only the first 352 bytes are read (of a .gz: inflated), where `load` -- and with it
    read_nii(only_header=True) -- inflates the whole file."""
    with _open(file_name, "rb") as f:
        raw = f.read(352)
    return _parse_header(raw, file_name)


def _header_bytes(shape, dtype, header):
    """The 352 bytes `save` writes in front of an array of `shape` (file order) and `dtype`."""
    dt = np.dtype(dtype)
    if dt not in _CODES:
        raise ValueError("unsupported dtype {}".format(dt))
    shape = [int(s) for s in shape]
    h = bytearray(352)
    struct.pack_into("<i", h, 0, 348)
    struct.pack_into("<8h", h, 40, *([len(shape)] + shape + [1] * (7 - len(shape))))
    struct.pack_into("<h", h, 70, _CODES[dt])
    struct.pack_into("<h", h, 72, dt.itemsize * 8)
    struct.pack_into("<8f", h, 76, *([header.qfac] + list(header.pixdim[:3]) + [1.0] * 4))
    struct.pack_into("<3f", h, 108, 352.0, header.scl_slope, header.scl_inter)
    struct.pack_into("<2h", h, 252, header.qform_code, 1 if header.sform is not None else 0)
    struct.pack_into("<3f", h, 256, *header.quatern)
    struct.pack_into("<3f", h, 268, *header.qoffset)
    if header.sform is not None:
        struct.pack_into("<12f", h, 280, *np.asarray(header.sform, np.float32).reshape(-1))
    h[344:348] = b"n+1\0"
    return bytes(h)


def save_flat(flat, shape, header, out_path, level=SAVE_GZIP_LEVEL):
    """`save` for data that is in file order already: `flat` is a dense 1-D array (file axis 0 fastest) of prod(shape)
    elements, written with `header`'s geometry behind the same 352 header bytes.  A .gz is written at `level` with mtime 0
    and no file name in the gzip header, so the bytes depend on the data alone."""
    flat = np.asarray(flat)
    if flat.ndim != 1 or not flat.flags.c_contiguous or flat.size != int(np.prod(shape)):
        raise ValueError("a dense 1-D array of {} elements expected, got shape {}".format(int(np.prod(shape)), flat.shape))
    if flat.dtype.byteorder == ">":
        raise ValueError("little-endian (or native) data expected")
    head = _header_bytes(shape, flat.dtype, header)
    out_path = str(out_path)
    with open(out_path, "wb") as raw:
        if out_path.endswith(".gz"):
            with gzip.GzipFile(filename="", mode="wb", compresslevel=level, fileobj=raw, mtime=0) as f:
                f.write(head)
                f.write(memoryview(flat).cast("B"))
        else:
            raw.write(head)
            raw.write(memoryview(flat).cast("B"))


def file_orientation(header, special=False):
    """What write_nii does to a (z, y, x) array on its way into a file with `header`: (trans_bk, (flip_x, flip_y, flip_z))
    -- file axis i runs along data axis trans_bk[i], after the flips; `special` (read_lits's x-mirrored cases) toggles the x
    flip, as two flips of one axis cancel."""
    affine = np.asarray(header.get_best_affine(), np.float64)
    if len(np.where(affine[:3, :3].reshape(-1) != 0)[0]) != 3:
        raise ValueError("an axis-aligned affine expected, got {}".format(affine[:3, :3].tolist()))
    trans, (flip_x, flip_y, flip_z) = _orient(affine)
    trans_bk = tuple(int(np.argwhere(np.array(trans[::-1]) == i)[0][0]) for i in range(3))
    if sorted(trans_bk) != [0, 1, 2]:
        raise ValueError("the affine {} does not name three different axes".format(affine[:3, :3].tolist()))
    return trans_bk, (bool(flip_x) != bool(special), bool(flip_y), bool(flip_z))


def data_shape(header):
    """(d, h, w) of the (z, y, x) array read_nii returns for a file with `header`."""
    trans_bk, _ = file_orientation(header)
    zyx = [0, 0, 0]
    for i, axis in enumerate(trans_bk):
        zyx[axis] = int(header.shape[i])
    return tuple(zyx)


def to_file_order(data, header, special=False, out_dtype=np.int16):
    """write_nii's flips, transpose and cast without the write: (z, y, x) data -> the flat array save_flat takes."""
    trans_bk, flips = file_orientation(header, special)
    for axis, flip in zip((2, 1, 0), flips):
        if flip:
            data = np.flip(data, axis=axis)
    return np.transpose(data, trans_bk).astype(out_dtype).reshape(-1, order="F")


PROB_LEVELS = 255           # --pred_type prob of the 3-D path: probabilities are stored as uint8 q = rint(255 p), scl_slope 1 / 255


def prob_header(header):
    """The header of a saved probability volume: `header`'s geometry with datatype uint8, scl_slope = 1 / 255 and
    scl_inter = 0, so any NIfTI reader (`load` included) returns q / 255 in [0, 1]."""
    import copy
    out = copy.copy(header)
    out.dtype = np.dtype(np.uint8)
    out.scl_slope, out.scl_inter = 1.0 / PROB_LEVELS, 0.0
    return out


def header_from_meta(size, spacing, dtype=np.int16):
    """A header for a case known only from meta.json (size = [d, h, w], spacing = [z, y, x]): pixdim (sx, sy, sz) and
    sform diag(-sx, -sy, +sz) with zero offsets -- the orientation read_nii returns unflipped, so the array index of the
    written file is (x, y, z) of the data."""
    d, h, w = (int(s) for s in size)
    sz, sy, sx = (float(s) for s in spacing)
    sform = np.zeros((3, 4), np.float64)
    sform[0, 0], sform[1, 1], sform[2, 2] = -sx, -sy, sz
    return Nifti1Header((w, h, d), dtype, (sx, sy, sz), sform=sform)
