"""No GPU: the host queries of the 3-D conv composition are the plan of the layer (csrc/conv3d.hip conv3d_plan).

unetk_conv3d_out_dims, unetk_conv3d_stat_rows(_bf16) and unetk_conv3d_ws_bytes(_bf16) each return one field of the plan the entry
points launch from, and all of it is pure host arithmetic.  The values are held to tests/golden/conv3d_plan_queries.npz, recorded
by tests/golden/make_conv3d_plan_fixture.py from the library as it was BEFORE the plan existed (every query then re-derived the
route on its own), for the extent sweep, the bf16 table and UNet3D's own layers: moving the queries onto the plan changed no
number.  A refused descriptor asks for 0 bytes and a negative row count, and is refused before the plan divides by a stride or
a channel count the descriptor could make zero.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_conv3d_plan_fixture", os.path.join(HERE, "golden", "make_conv3d_plan_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_generator()
GROUPS = G.groups()
NAMES = list(GROUPS)
E_BADARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    return G.library()


@pytest.fixture(scope="module")
def recorded():
    z = np.load(G.OUT)
    assert list(z["names"]) == NAMES
    return {name: (z["desc_%02d" % i], z["values_%02d" % i]) for i, name in enumerate(NAMES)}


def test_fixture_is_small_and_covers_every_layer_family():
    assert os.path.getsize(G.OUT) < 100 * 1024
    assert sum(len(v) for v in GROUPS.values()) >= 2790 + 15 + 4 * 18
    for name in ("unet3d 96^3", "unet3d 10x256x256"):
        layers = GROUPS[name]
        assert {(t.kd, t.sd, t.shw) for t in layers} == {(1, 1, 1), (1, 1, 2), (3, 1, 1), (3, 1, 2), (3, 2, 2)}
        # the padded levels carry masks: 240 of 256 channels, and the concat of two such halves
        assert any(t.cin == 512 and t.cin_live == ((1 << 30) - 1) * ((1 << 32) + 1) for t in layers)
        assert any(t.cout == 256 and t.cout_live == (1 << 30) - 1 for t in layers)
        assert any(t.ys == 2 * t.cout for t in layers) and any(t.xs == 2 * t.cin for t in layers)


@pytest.mark.parametrize("name", NAMES)
def test_queries_equal_the_values_recorded_before_the_plan(L, recorded, name):
    descs, (rdesc, rvalues) = GROUPS[name], recorded[name]
    assert np.array_equal(np.array(descs, dtype=np.int64), rdesc), "the fixture was recorded for another descriptor list"
    bad = []
    for t, want in zip(descs, rvalues.tolist()):
        got = G.ask(L, t)
        if list(got) != want:
            bad.append((tuple(t), dict(zip(G.VALUES, got)), dict(zip(G.VALUES, want))))
    assert not bad, "{} of {} descriptors, the first: {}".format(len(bad), len(descs), bad[:3])


def test_recorded_values_are_not_trivial(recorded):
    """Nothing of the fp32 queries is refused; the bf16 queries answer inside the layer rule and refuse outside it."""
    for name in NAMES:
        rdesc, v = recorded[name]
        col = {k: v[:, i] for i, k in enumerate(G.VALUES)}
        assert (col["rc"] == 0).all() and (col["stat_rows"] > 0).all()
        rule = (rdesc[:, 7] == 1) & (rdesc[:, 8] == 1) & (rdesc[:, 4] % 32 == 0) & (rdesc[:, 5] % 32 == 0)
        assert ((col["stat_rows_bf16"] > 0) == rule).all() and ((col["ws_bytes_bf16"] > 0) == rule).all()
        assert (col["stat_rows_bf16"][~rule] == E_UNSUPPORTED).all()
        s2 = rdesc[:, 8] == 2
        assert (col["ws_bytes"][s2] > 0).all()


# (kd, sd, shw): kernel depths and strides no layer has, a zero stride included (the output extents divide by it), and the
# depth-strided (1,3,3) kernel
BAD_FAMILIES = [(2, 1, 1), (0, 1, 1), (3, 3, 1), (3, 1, 3), (3, 0, 1), (3, 1, 0), (1, 0, 0), (3, -1, 2), (1, 2, 1), (1, 2, 2)]


@pytest.mark.parametrize("kd,sd,shw", BAD_FAMILIES, ids=["k{}s{}{}".format(*f) for f in BAD_FAMILIES])
def test_bad_kernel_depth_or_stride_is_refused_before_the_plan_divides(L, kd, sd, shw):
    for cin, cout in ((64, 64), (32, 128), (30, 30)):
        for d, h, w in ((4, 8, 8), (1, 1, 1), (5, 24, 24)):
            got = dict(zip(G.VALUES, G.ask(L, G.Desc(2, d, h, w, cin, cout, kd, sd, shw, cin, cout, 0, 0))))
            assert got["rc"] == E_BADARG and (got["do"], got["ho"], got["wo"]) == (-1, -1, -1), got
            assert got["stat_rows"] == E_BADARG and got["stat_rows_bf16"] == E_BADARG, got
            assert got["ws_bytes"] == 0 and got["ws_bytes_bf16"] == 0, got


ZEROS = [dict(n=0), dict(d=0), dict(h=0), dict(w=0), dict(cin=0, xs=0), dict(cout=0, ys=0), dict(xs=32), dict(ys=32)]


@pytest.mark.parametrize("edit", ZEROS, ids=["-".join(sorted(e)) for e in ZEROS])
def test_empty_extent_or_short_stride_is_refused_before_the_plan_divides(L, edit):
    for kd, (sd, shw, _) in ((1, (1, 1, 1)), (3, (1, 2, 2)), (3, (2, 2, 2))):
        got = dict(zip(G.VALUES, G.ask(L, G.Desc(2, 4, 8, 8, 64, 64, kd, sd, shw, 64, 64, 0, 0)._replace(**edit))))
        assert got["rc"] == E_BADARG and got["stat_rows"] == E_BADARG and got["stat_rows_bf16"] == E_BADARG, got
        assert got["ws_bytes"] == 0 and got["ws_bytes_bf16"] == 0, got


# outside the bf16 layer rule (include/unetk.h: stride 1, Cin % 32 == 0, Cout % 32 == 0): (kd, sd, shw, Cin, Cout)
OUTSIDE_RULE = [(3, 1, 2, 64, 64), (3, 2, 2, 64, 64), (1, 1, 2, 64, 64), (3, 2, 1, 64, 64), (3, 1, 1, 48, 64), (1, 1, 1, 64, 48),
                (3, 1, 1, 1, 32), (1, 1, 1, 30, 30)]


@pytest.mark.parametrize("kd,sd,shw,cin,cout", OUTSIDE_RULE, ids=["k{}s{}{}-{}x{}".format(*r) for r in OUTSIDE_RULE])
def test_bf16_request_outside_the_layer_rule_asks_for_nothing(L, kd, sd, shw, cin, cout):
    for d, h, w in ((4, 8, 8), (1, 1, 1), (6, 24, 24)):
        got = dict(zip(G.VALUES, G.ask(L, G.Desc(1, d, h, w, cin, cout, kd, sd, shw, cin, cout, 0, 0))))
        assert got["stat_rows_bf16"] == E_UNSUPPORTED and got["ws_bytes_bf16"] == 0, got
        assert got["rc"] == 0 and got["stat_rows"] > 0, got      # the fp32 queries answer: the descriptor itself is fine
