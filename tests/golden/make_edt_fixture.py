"""Records the 3-D boundary-weight map (csrc/weights.hip): tests/golden/edt_maps_before.npz.

Run once on a GPU, at the commit before b3_x_kernel and b3_axis_kernel were moved onto csrc/edt_int.h:
    python tests/golden/make_edt_fixture.py
It asks whatever library UNETK_LIB names (default: the tree's own), through `ops.boundary_weights3d` only, for the float32 bits of
the map of `boundary3d_ref.labels(shape, 100 + sum(shape), n=2)` at every shape of SHAPES and every z scale of SCALES:

  (3, 9, 65)   a second ballot word of the x pass and a second 64-column strip of the axis passes
  (17, 5, 6)   a second block of 16 outputs along z
  (129, 3, 4)  a second staging chunk of 128 rows along z

test_gpu_boundary3d.py::test_map_bits_are_those_before_the_shared_edt_core imports SHAPES, SCALES, `key` and `record` from here
and holds the library to the recorded bits.  The map is the last thing the passes compute (integer minima, sqrt, expf, the double
sums in their fixed order, the float32 scale): any change to one of them shows in its bits.  The integer fields need no recording,
they compare exactly with scipy (test_exact_rows).  The archive is written with fixed member dates, so a rerun against a library
that answers the same reproduces the file byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import boundary3d_ref as bref  # noqa: E402

OUT = os.path.join(HERE, "edt_maps_before.npz")
SHAPES = ((3, 9, 65), (17, 5, 6), (129, 3, 4))
SCALES = (1, 3)


def key(shape, k):
    return "map_{}_k{}".format("x".join(str(v) for v in shape), k)


def volume(shape):
    return bref.labels(shape, 100 + sum(shape), n=2)


def record(ops, shape, k):
    """uint32 [2, D, H, W]: the bits of the map."""
    import torch
    wmap = ops.boundary_weights3d(torch.from_numpy(volume(shape)).cuda(), k)
    torch.cuda.synchronize()
    return wmap.cpu().numpy().view(np.uint32)


def write_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main(out=OUT):
    from boxsegliver_amd import ops
    arrays = [(key(s, k), record(ops, s, k)) for s in SHAPES for k in SCALES]
    for name, a in arrays:
        f = a.view(np.float32)
        assert np.isfinite(f).all() and f.min() >= 0.5 and (f != 1.0).any(), name      # a real map, not a ring-free one
    write_npz(out, arrays)
    print("{}: {} maps, {} values, {} bytes".format(out, len(arrays), sum(a.size for _, a in arrays), os.path.getsize(out)))


if __name__ == "__main__":
    main(*sys.argv[1:2])
