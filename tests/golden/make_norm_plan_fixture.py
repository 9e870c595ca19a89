"""Records the two host queries of the normaliser family (csrc/norm.hip): tests/golden/norm_plan_queries.npz.

Run once, at the commit before the entry points were moved onto NormPlan:  python tests/golden/make_norm_plan_fixture.py
It asks whatever library UNETK_LIB names (default: the tree's own).  test_norm_plan_host.py imports the sweep and `ask_*` from
here and holds the library to the recorded values of

  * unetk_norm_bwd_ws_bytes        over N x HW x C x per_sample x guide_ch x storage                       -> bwd [5,6,9,2,5,2]
  * unetk_norm_finalize_ws_bytes   over the same descriptors and stat_rows = Ns x {1, 64, 256, 257, 1025}  -> fin [5,6,9,2,5,2,5]

Both are pure host arithmetic: no GPU.  The archive is written with fixed member dates, so a rerun against a library that answers
the same reproduces the file byte for byte."""
import ctypes
import io
import itertools
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "norm_plan_queries.npz")
FP32S, BF16S = 0, 2
AXES = (("N", (1, 2, 3, 5, 32)), ("HW", (1, 16, 100, 4096, 65536, 884736)), ("C", (4, 8, 24, 64, 96, 200, 516, 1000, 1024)),
        ("per_sample", (0, 1)), ("guide_ch", (0, 1, 2, 3, 4)), ("storage", (FP32S, BF16S)))
ROW_FACTORS = (1, 64, 256, 257, 1025)          # stat_rows = factor x Ns: the reducer's direct route ends at 256 rows per group
SHAPE = tuple(len(v) for _, v in AXES)


def sweep():
    """Every (N, HW, C, per_sample, guide_ch, storage) in the order of the recorded arrays."""
    return itertools.product(*(v for _, v in AXES))


def desc(n, hw, c, ps, g, st, **over):
    """A plain descriptor of the sweep's six coordinates; `over` replaces fields by their names in unetk_norm_desc."""
    from boxsegliver_amd import _abi
    f = dict(N=n, HW=hw, C=c, per_sample=ps, z_stride=c, guide_ch=g, gw_stride=c if g else 0, gw_coff=0, affine_only=0,
             guide_leaky=0, storage=st, guide_alpha=0.0, dropout_keep=0.0, dropout_seed=0, guide_per_sample=0)
    f.update(over)
    return _abi.NormDesc(*(f[k] for k, _ in _abi.NormDesc._fields_))


def library():
    from boxsegliver_amd import _abi
    lib = _abi.lib()
    lib.unetk_norm_bwd_ws_bytes.restype = ctypes.c_size_t
    lib.unetk_norm_finalize_ws_bytes.restype = ctypes.c_size_t
    return lib


def ask_bwd(lib, d):
    return int(lib.unetk_norm_bwd_ws_bytes(ctypes.byref(d)))


def ask_finalize(lib, d, stat_rows):
    return int(lib.unetk_norm_finalize_ws_bytes(ctypes.byref(d), int(stat_rows)))


def record(lib):
    bwd, fin = [], []
    for t in sweep():
        d = desc(*t)
        ns = t[0] if t[3] else 1
        bwd.append(ask_bwd(lib, d))
        fin.append([ask_finalize(lib, d, k * ns) for k in ROW_FACTORS])
    return (np.array(bwd, dtype=np.int64).reshape(SHAPE), np.array(fin, dtype=np.int64).reshape(SHAPE + (len(ROW_FACTORS),)))


def write_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    bwd, fin = record(library())
    write_npz(OUT, [("bwd", bwd), ("fin", fin)] + [("axis_" + k, np.array(v, dtype=np.int64)) for k, v in AXES] +
              [("row_factors", np.array(ROW_FACTORS, dtype=np.int64))])
    print("{}: {} + {} values, {} bytes".format(OUT, bwd.size, fin.size, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
