"""The optimiser kernels (csrc/optim.hip) past their grid caps and with every option, against float64.

The reference is TF's update formulas as oracle/solver.py states them (epsilon outside the bias correction; momentum's
accum = mom * accum + g, Nesterov step lr * (g + mom * accum)), with the l2 regulariser's gradient l2 * p added to the scaled
gradient and AdamW's var <- var * (1 - wd) before the Adam update, run for 5 steps in float64: numpy for the small sizes, the
same function on float64 device tensors for the large ones.  It is cross-checked against oracle.solver's classes below.
Bounds: rtol 2e-5, atol 2e-6 on p, m, v / accum as in test_gpu_ops.py::test_adam_and_momentum_match_tf_formulas; sumsq 1e-6
relative as in test_sumsq_sizes_and_alignment.
"""
import math

import numpy as np
import pytest
import torch

from oracle import solver as osolver

pytestmark = pytest.mark.gpu

STEPS = 5
B1, B2, EPS, LR = 0.9, 0.99, 1e-8, 1e-3
RTOL, ATOL = 2e-5, 2e-6
ADAM_GRID_CAP = 8192 * 256 * 4            # elements one pass of adam_kernel's capped grid covers (float4 per thread)
FLAT_GRID_CAP = 8192 * 256                # momentum_kernel: one element per thread
SUMSQ_GRID_CAP = 1024 * 256 * 4


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def adam_ref(p, m, v, g, lr_t, gscale, l2, dwd):
    """One TF Adam / AdamW step on float64 arrays (numpy or torch); returns the new p, m, v."""
    gg = l2 * p + g * gscale
    m = m + (1 - B1) * (gg - m)
    v = v + (1 - B2) * (gg * gg - v)
    return p * (1 - dwd) - lr_t * m / (v ** 0.5 + EPS), m, v


def momentum_ref(p, acc, g, lr, mom, nesterov, gscale, l2):
    gg = l2 * p + g * gscale
    acc = mom * acc + gg
    return p - (lr * (gg + mom * acc) if nesterov else lr * acc), acc


def lr_t_of(t):
    return LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)


def _close(got, ref, what):
    if isinstance(ref, np.ndarray):
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=ATOL, err_msg=what)
    else:
        err = (got.double() - ref).abs() - RTOL * ref.abs()
        assert err.max().item() <= ATOL, (what, err.max().item())


def _f64(t, on_device):
    return t.double() if on_device else t.double().cpu().numpy()


def test_restatements_agree_with_oracle_solver():
    rng = np.random.default_rng(3)
    n, wd = 1003, 1e-2
    p0 = rng.standard_normal(n)
    for nesterov in (False, True):
        pa, pm = {"w": p0.copy()}, {"w": p0.copy()}
        adam, mom = osolver.TFAdam(B1, B2, EPS), osolver.TFMomentum(0.9, nesterov)
        p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
        q, acc = p0.copy(), np.zeros(n)
        for t in range(1, STEPS + 1):
            g = rng.standard_normal(n)
            adam.step(pa, {"w": 0.5 * g + wd * pa["w"]}, LR)
            mom.step(pm, {"w": 0.5 * g + wd * pm["w"]}, 0.1)
            p, m, v = adam_ref(p, m, v, g, lr_t_of(t), 0.5, wd, 0.0)
            q, acc = momentum_ref(q, acc, g, 0.1, 0.9, nesterov, 0.5, wd)
        np.testing.assert_allclose(p, pa["w"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(q, pm["w"], rtol=1e-12, atol=1e-14)


ADAM_OPTS = [("l2_gscale", 0.5, 1e-2, 0.0), ("adamw", 1.0, 0.0, 0.05), ("l2_gscale_adamw", 0.5, 1e-2, 0.05)]
ADAM_SIZES = [1, 3, 4, 1003, ADAM_GRID_CAP + 5, 31000003]


@pytest.mark.parametrize("opt", ADAM_OPTS, ids=[o[0] for o in ADAM_OPTS])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_sizes_and_options(ops, n, opt):
    """n = 1, 3 (tail only), 4 (body only), 1003, one pass of the capped grid plus a tail, and the real buffer's order."""
    _, gscale, l2, dwd = opt
    on_device = n > (1 << 16)
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + 7)
    p = torch.randn(n, device="cuda", generator=gen)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    rp, rm, rv = _f64(p, on_device), _f64(m, on_device), _f64(v, on_device)
    for t in range(1, STEPS + 1):
        g = torch.randn(n, device="cuda", generator=gen)
        rp, rm, rv = adam_ref(rp, rm, rv, _f64(g, on_device), lr_t_of(t), gscale, l2, dwd)
        ops.adam_step(p, g, m, v, lr_t_of(t), B1, B2, EPS, gscale, l2, dwd)
    _close(p, rp, "p")
    _close(m, rm, "m")
    _close(v, rv, "v")


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
def test_adam_refuses_a_misaligned_view_and_leaves_the_state(ops, which):
    from boxsegliver_amd import _abi
    n = 1003
    gen = torch.Generator(device="cuda").manual_seed(11)
    bufs = {k: torch.randn(n + 8, device="cuda", generator=gen) for k in "pgmv"}
    bufs["v"].abs_()
    snap = {k: t.clone() for k, t in bufs.items()}
    views = {k: t[1:1 + n] if k == which else t[:n] for k, t in bufs.items()}
    with pytest.raises(_abi.UnetkError, match=r"\(code -1\)"):
        ops.adam_step(views["p"], views["g"], views["m"], views["v"], LR, B1, B2, EPS, 0.5, 1e-2, 0.05)
    torch.cuda.synchronize()
    for k in "pgmv":
        assert torch.equal(bufs[k], snap[k]), k


MOM_OPTS = [("plain", 1.0, 0.0), ("l2_gscale", 0.5, 1e-2)]


@pytest.mark.parametrize("opt", MOM_OPTS, ids=[o[0] for o in MOM_OPTS])
@pytest.mark.parametrize("nesterov", [False, True], ids=["heavy_ball", "nesterov"])
@pytest.mark.parametrize("n", [1, 1003, FLAT_GRID_CAP + 77])
def test_momentum_sizes_and_options(ops, n, nesterov, opt):
    _, gscale, l2 = opt
    on_device = n > (1 << 16)
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + 13)
    p = torch.randn(n, device="cuda", generator=gen)
    acc = torch.zeros(n, device="cuda")
    rp, ra = _f64(p, on_device), _f64(acc, on_device)
    for _ in range(STEPS):
        g = torch.randn(n, device="cuda", generator=gen)
        rp, ra = momentum_ref(rp, ra, _f64(g, on_device), 0.1, 0.9, nesterov, gscale, l2)
        ops.momentum_step(p, g, acc, 0.1, 0.9, nesterov, gscale, l2)
    _close(p, rp, "p")
    _close(acc, ra, "accum")


@pytest.mark.parametrize("n,off", [(SUMSQ_GRID_CAP + 5, 0), (SUMSQ_GRID_CAP + 5, 1), (5000003, 2), (31000001, 0), (31000001, 3)])
def test_sumsq_past_the_block_clamp(ops, n, off):
    """More than 1024 blocks' worth: the strided float4 body and its tail; a view off a 16-byte boundary takes the scalar loop."""
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + off)
    buf = torch.randn(n + 8, device="cuda", generator=gen)
    v = buf[off:off + n]
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    ref = float((v.double() ** 2).sum())
    got = float(ops.sumsq(v).item())
    assert abs(got - ref) <= 1e-6 * max(ref, 1.0), (got, ref)
    assert got == float(ops.sumsq(v).item())                 # fixed summation order
