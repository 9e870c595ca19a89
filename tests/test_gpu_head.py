"""The loss head (csrc/head.hip) on every dispatch path, against a float64 restatement of the reference's formulas.

The restatement (head_ref) follows loss_metrics.py:115-231 the way oracle/losses.py does, but keeps every step in float64:
logits = z @ w + b, softmax, the class / pixel weights of each mode with their per-sample renormalisation to mean 1,
tf.losses' SUM_BY_NONZERO_WEIGHTS, the soft Dice without background (eps 1e-8) and the metric sums on p > 0.5.  Gradients come
from autograd on it.  Small cases evaluate it on the CPU, the multi-million-pixel ones on the device (same code).

Each row of CASES names the path it exists to reach -- blocks per sample and whether the cap clamped them, the backward's
block count and the row-reduce route of dw / db -- and the test recomputes those from head_ws()'s formulas (and the whole
workspace size, which must equal unetk_head_ws_bytes) so that a row that lands elsewhere fails.

Bounds: every row keeps test_gpu_ops.py::test_head_forward_backward's (3e-6 relative on logits, 2e-6 absolute on
probabilities, 2e-5 on losses, I / U and gradients).  A row that float32 arithmetic alone kept from those would carry a `tol`
override of 4 x the error of this same restatement evaluated in torch float32 on the CPU against its float64 self on that
row's inputs.  That was measured for every row: gradients <= 4.3e-6, losses and I / U <= 1.9e-7, logits <= 5.7e-7; the
probabilities of the C = 128 / 256 rows (1.1e-6, 2.1e-6) and of the large-logit rows (5.4e-6, 1.5e-6) would qualify for
4.4e-6 / 8.4e-6 / 2.2e-5 / 6.0e-6, but no row claims an override: every row is held to the plain bounds.
"""
import collections
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import losses as olosses

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -2
NUMERIC_W = [0.2, 0.4, 0.0, 4.4, 0.7, 2.0, 0.3, 1.5]      # a zero weight (class 2) leaves the denominator
DECAY = 1000.0
BWD_COMBOS = [(1.0, 0.0, None), (0.0, 1.0, (1.0, 1.0)), (0.7, 0.3, (0.5, 2.0))]     # xent_scale, dice_scale, dev_scales
TOL = {"logits": 3e-6, "probs": 2e-6, "loss": 2e-5, "grad": 2e-5}


@pytest.fixture(scope="module")
def ops():
    from boxsegliver_amd import ops as _ops
    from boxsegliver_amd import _abi
    _abi.lib()
    return _ops


def lib():
    from boxsegliver_amd import _abi
    return _abi.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def numeric_w(ncls):
    return [0.0, 1.0] if ncls == 2 else NUMERIC_W[:ncls]


def class_weights(mode, onehot, nw=None, decay=None):
    """loss_metrics.py:115-165 on a one-hot [N, HW, ncls] of any float type: per-pixel weights [N, HW], renormalised per sample
    to mean 1 (the plain 1.0 of `none` is returned as ones)."""
    n, hw, ncls = onehot.shape
    if mode == "none":
        return torch.ones((n, hw), dtype=onehot.dtype, device=onehot.device)
    if mode == "numerical":
        w = (onehot * torch.tensor(nw, dtype=onehot.dtype, device=onehot.device)).sum(-1)
    elif mode == "proportion":
        num = onehot.sum(1)
        if decay:
            num = num + decay
        prop = 1.0 / num
        pw = prop / prop.sum(1, keepdim=True)
        w = (onehot * pw[:, None, :]).sum(-1)
    else:
        raise ValueError(mode)
    return w / w.sum(1, keepdim=True) * float(hw)


def head_ref(z, w, b, labels, mode, nw=None, decay=None, pixel_w=None, dtype=torch.float64, device="cpu", grads=True):
    """z [N, HW, C], w [C, ncls], b [ncls], labels [N, HW] -> dict of everything the kernels produce, in `dtype`."""
    z = z.to(device=device, dtype=dtype).requires_grad_(grads)
    w = w.to(device=device, dtype=dtype).requires_grad_(grads)
    b = b.to(device=device, dtype=dtype).requires_grad_(grads)
    labels = labels.to(device=device, dtype=torch.int64)
    n, hw, _ = z.shape
    ncls = w.shape[1]
    logits = z @ w + b
    probs = torch.softmax(logits, -1)
    onehot = F.one_hot(labels, ncls).to(dtype)
    ce = -(torch.log_softmax(logits, -1) * onehot).sum(-1)
    if mode == "pixelmap":
        wt = pixel_w.to(device=device, dtype=dtype)
    else:
        wt = class_weights(mode, onehot, nw, decay)
    present = (wt != 0).sum().to(dtype)
    total = (ce * wt).sum()
    xent = total / present if present.item() > 0 else total * 0.0            # tf.losses: div_no_nan(total, num_present)
    oh, pf = onehot[..., 1:], probs[..., 1:]
    inter, union = (oh * pf).sum((1, 2)), (oh + pf).sum((1, 2))
    dice = 1.0 - ((2.0 * inter) / (union + 1e-8)).mean()
    out = {"logits": logits.detach(), "probs": probs.detach(), "xent": xent.item(), "dice": dice.item(),
           "present": present.item(), "iu": torch.stack([inter, union], 1).detach()}
    # metric sums on p > 0.5, as a bracket: a pixel within 1e-5 of the threshold may fall either way
    pd = probs.detach()[..., 1:]
    amb = (pd - 0.5).abs() <= 1e-5
    out["ambiguous"] = amb.double().mean().item()
    for name, pr in (("lo", (pd > 0.5) & ~amb), ("hi", (pd > 0.5) | amb)):
        pr = pr.to(dtype)
        ohd = oh.detach()
        out[name] = torch.stack([(pr * ohd).sum(1), pr.sum(1), ohd.sum(1), (pr + ohd).clamp(0, 1).sum(1)], -1)   # [N, ncls-1, 4]
    if grads:
        out["gx"] = torch.autograd.grad(xent, (z, w, b), retain_graph=True, allow_unused=True)
        out["gd"] = torch.autograd.grad(dice, (z, w, b))
    return out


# ------------------------------------------------------------------------------------------------ head_ws()'s formulas
def head_paths(n, hw, c, ncls):
    cap = 64 if n >= 32 else (2048 + n - 1) // n
    want = (hw + 1023) // 1024
    bps = max(1, min(want, cap))
    npix = n * hw
    nblk = min((npix + 255) // 256, 2048)
    route = "direct" if nblk <= 256 else ("wide" if nblk <= 1024 else "two_level")
    nq = 2 + (ncls - 1) * 6
    r4 = lambda v: (v + 3) & ~3
    off = r4(2 * n * ncls)
    off = r4(off + n * bps * nq)
    off = r4(off + nblk * c * ncls + nblk * ncls)
    off += 64 * c * ncls if nblk > 256 else 0
    return {"bps": bps, "clamped": (want > cap) and ("n>=32" if n >= 32 else "n<32"), "nblk": nblk, "route": route,
            "stride": npix > 2048 * 256, "ws_bytes": off * 4}


Case = collections.namedtuple("Case", "id n hw c ncls mode labels scale storage expect tol")


def _case(id, n, hw, c, ncls, mode, expect, labels="random", scale="o1", storage="fp32", tol=None):
    return Case(id, n, hw, c, ncls, mode, labels, scale, storage, expect, dict(TOL, **(tol or {})))


def _e(bps, nblk, route, clamped=False, stride=False):
    return {"bps": bps, "clamped": clamped, "nblk": nblk, "route": route, "stride": stride}


CASES = [
    # ---- O(1) logits, fp32: channel widths (lanes per pixel 1..64), class counts 2..8, HW edges, N = 1, 2, 7, 33
    _case("c4_hw1_n7_k2", 7, 1, 4, 2, "none", _e(1, 1, "direct")),                           # lpp 1: the step-1 pixel loop
    _case("c8_hw3_n2_k8", 2, 3, 8, 8, "numerical", _e(1, 1, "direct")),                      # lpp 2, HW = lpp + 1
    _case("c64_hw15_n33_k3", 33, 15, 64, 3, "proportion", _e(1, 2, "direct")),               # DPP branch, HW = lpp - 1
    _case("c32_hw9_n2_k2", 2, 9, 32, 2, "pixelmap", _e(1, 1, "direct")),                     # shuffle branch, HW = lpp + 1
    _case("c16_hw255_n3_k4", 3, 255, 16, 4, "numerical", _e(1, 3, "direct"), labels="degenerate"),
    _case("c32_hw1024_n7_k5", 7, 1024, 32, 5, "proportion", _e(1, 28, "direct"), labels="degenerate"),
    _case("c64_hw1025_n2_k3", 2, 1025, 64, 3, "pixelmap", _e(2, 9, "direct")),
    _case("c128_hw4099_n2_k6", 2, 4099, 128, 6, "none", _e(5, 33, "direct"), labels="degenerate"),
    _case("c256_hw4099_n1_k7", 1, 4099, 256, 7, "numerical", _e(5, 17, "direct")),
    _case("c64_hw1024_n3_k3_map0", 3, 1024, 64, 3, "pixelmap0", _e(1, 12, "direct")),        # num_present = 0
    # ---- several blocks per sample, L > 1 finalisation slices, the three row-reduce routes of dw / db
    _case("c16_hw50000_n2_k3", 2, 50000, 16, 3, "numerical", _e(49, 391, "wide")),           # db (ncls 3): two levels
    _case("c8_hw100000_n1_k4", 1, 100000, 8, 4, "proportion", _e(98, 391, "wide")),          # db (ncls 4): float4 direct
    _case("c4_hw50000_n7_k2", 7, 50000, 4, 2, "none", _e(49, 1368, "two_level"), labels="degenerate"),
    _case("c4_hw2100000_n1_k8", 1, 2100000, 4, 8, "proportion", _e(2048, 2048, "two_level", "n<32", True)),
    _case("c8_hw66000_n33_k3", 33, 66000, 8, 3, "numerical", _e(64, 2048, "two_level", "n>=32", True)),
    # ---- large logits (|logit| reaches about 100): expf underflows to 0, probabilities are exactly 0 and 1
    _case("big_c64_hw1024_n2_k3", 2, 1024, 64, 3, "none", _e(1, 8, "direct"), scale="big"),
    # sample 0: no foreground AND background logits ~200 above the others: every foreground probability underflows to exactly 0,
    # Dice I = U = 0, only the 1e-8 keeps the backward's 1 / U^2 finite (its gradient there is exactly 0)
    _case("bgsure_c64_hw255_n3_k3", 3, 255, 64, 3, "none", _e(1, 3, "direct"), labels="bg_certain"),
    _case("big_c32_hw255_n2_k2", 2, 255, 32, 2, "numerical", _e(1, 2, "direct"), scale="big"),
    # ---- bf16 storage of z and dz
    _case("bf16_c64_hw1025_n2_k3", 2, 1025, 64, 3, "numerical", _e(2, 9, "direct"), storage="bf16"),
    _case("bf16_c32_hw255_n7_k2", 7, 255, 32, 2, "proportion", _e(1, 7, "direct"), storage="bf16", labels="degenerate"),
    _case("bf16_c8_hw3_n2_k8", 2, 3, 8, 8, "none", _e(1, 1, "direct"), storage="bf16"),
    _case("bf16_c16_hw50000_n2_k3", 2, 50000, 16, 3, "pixelmap", _e(49, 391, "wide"), storage="bf16"),
    # ---- batches beyond one pass of head_finalize_kernel's 64 KiB of LDS (264 samples of 3 classes, 90 of 8, 431 of 2)
    _case("n512_c16_hw64_k3", 512, 64, 16, 3, "numerical", _e(1, 128, "direct")),
    _case("n128_c16_hw64_k8", 128, 64, 16, 8, "proportion", _e(1, 32, "direct")),
    _case("n2048_c16_hw16_k2", 2048, 16, 16, 2, "none", _e(1, 128, "direct")),
]


def make_inputs(case):
    """Seeded CPU tensors of a case: z [N, HW, C] (fp32, or the bf16 values the kernel reads), w, b, labels, pixel map."""
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in case.id))
    n, hw, c, ncls = case.n, case.hw, case.c, case.ncls
    z = torch.randn((n, hw, c), generator=g)
    wscale = 0.3 if case.scale == "o1" else 25.0 / math.sqrt(c)
    w = torch.randn((c, ncls), generator=g) * wscale
    b = torch.randn(ncls, generator=g) * 0.1
    labels = torch.randint(0, ncls, (n, hw), generator=g, dtype=torch.int32)
    if case.labels == "degenerate":
        labels[0] = 0                                      # no foreground: Dice I = 0, U = sum p
        labels[1] = 1                                      # all one foreground class
        if n > 2:
            labels[2][labels[2] == ncls - 1] = 0           # a class absent from a sample
    if case.labels == "bg_certain":
        labels[0] = 0
        z[0] = 40.0 * w[:, 0]
    pixel_w = None
    if case.mode == "pixelmap":
        pixel_w = torch.rand((n, hw), generator=g) + 0.5
        pixel_w[torch.rand((n, hw), generator=g) < 0.3] = 0.0
        pixel_w[:, 0] = 1.0
        pixel_w = pixel_w / pixel_w.sum(1, keepdim=True) * float(hw)
    elif case.mode == "pixelmap0":
        pixel_w = torch.zeros((n, hw))
    if case.storage == "bf16":
        z = z.bfloat16()
    return z, w, b, labels, pixel_w


def ref_of(case, inputs, dtype=torch.float64, device=None):
    z, w, b, labels, pixel_w = inputs
    if device is None:
        device = "cpu" if z.numel() <= (1 << 21) else "cuda"
    mode = "pixelmap" if case.mode.startswith("pixelmap") else case.mode
    return head_ref(z, w, b, labels, mode, numeric_w(case.ncls), DECAY if mode == "proportion" else None, pixel_w, dtype, device)


def desc_of(ops, case):
    mode = "pixelmap" if case.mode.startswith("pixelmap") else case.mode
    return ops.head_desc(case.n, case.hw, case.c, case.ncls, mode, numeric_w=numeric_w(case.ncls) if mode == "numerical" else None,
                         proportion_decay=DECAY if mode == "proportion" else 0.0)


def rel_err(got, ref):
    got, ref = got.double(), ref.double().to(got.device)
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _stored_ok(got_bf16, ref64, flips):
    from test_gpu_bf16s import _stored_ok as ok
    ok(got_bf16, ref64, flips=flips)


def split_result(res, n, ncls):
    m = n * (ncls - 1) * 4
    return res[:3], res[3:3 + m].reshape(n, ncls - 1, 4), res[3 + m:].reshape(n, 2)


def check_counts(sums, ref):
    """Each kernel count between the reference count with the ambiguous pixels off and with them on."""
    assert ref["ambiguous"] <= 1e-3, ref["ambiguous"]
    sums = sums.double().cpu()
    lo, hi = ref["lo"].double().cpu(), ref["hi"].double().cpu()
    assert bool(((sums >= lo) & (sums <= hi)).all()), ((sums - lo).min().item(), (hi - sums).min().item())


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_head_paths_against_float64(ops, case):
    n, hw, c, ncls = case.n, case.hw, case.c, case.ncls
    tol = case.tol
    d = desc_of(ops, case)
    paths = head_paths(n, hw, c, ncls)
    assert {k: paths[k] for k in case.expect} == case.expect                 # the path this row exists for
    assert lib().unetk_head_ws_bytes(ctypes.byref(d)) == paths["ws_bytes"]
    inputs = make_inputs(case)
    ref = ref_of(case, inputs)
    z, w, b, labels, pixel_w = [None if t is None else t.cuda() for t in inputs]
    zd = z.reshape(n * hw, c).contiguous()

    def run():
        lg, probs, result, ws = ops.head_fwd(d, zd, w, b, labels, pixel_w, want_probs=True)
        outs = [lg, probs, result]
        for xs, ds, sc in BWD_COMBOS:
            scales = None if sc is None else torch.tensor(sc, device="cuda")
            outs += list(ops.head_bwd(d, zd, w, labels, pixel_w, lg, result, ws, xs, ds, scales))
        torch.cuda.synchronize()
        return outs

    first, again = run(), run()
    for k, (a, bb) in enumerate(zip(first, again)):
        assert torch.equal(_bits(a), _bits(bb)), "output {} differs between two runs".format(k)
    lg, probs, result = first[:3]
    head3, sums, iu = split_result(result.cpu().double(), n, ncls)
    figures = {"logits": rel_err(lg.reshape(n, hw, ncls), ref["logits"]),
               "probs": (probs.reshape(n, hw, ncls).double() - ref["probs"].to(probs.device)).abs().max().item(),
               "xent": abs(head3[0].item() - ref["xent"]) / max(1.0, abs(ref["xent"])),
               "dice": abs(head3[1].item() - ref["dice"]) / max(1.0, abs(ref["dice"])),
               "iu": ((iu - ref["iu"].cpu()).abs() / ref["iu"].cpu().abs().clamp_min(1.0)).max().item()}
    print(case.id, " ".join("{} {:.2e}".format(k, v) for k, v in figures.items()))
    assert figures["logits"] < tol["logits"]
    assert figures["probs"] < tol["probs"]
    assert figures["xent"] < tol["loss"] and figures["dice"] < tol["loss"] and figures["iu"] < tol["loss"]
    assert head3[2].item() == ref["present"]
    if case.mode == "pixelmap0":
        assert head3[0].item() == 0.0 and head3[2].item() == 0.0
    if case.labels == "bg_certain":
        assert iu[0, 0].item() == 0.0 and iu[0, 1].item() == 0.0 and ref["iu"][0, 1].item() < 1e-30
    check_counts(sums, ref)
    for k, (xs, ds, sc) in enumerate(BWD_COMBOS):
        dz, dw, db = first[3 + 3 * k:6 + 3 * k]
        s0, s1 = (1.0, 1.0) if sc is None else sc
        exp = [xs * s0 * (gx if gx is not None else 0.0) + ds * s1 * gd for gx, gd in zip(ref["gx"], ref["gd"])]
        if case.mode == "pixelmap0" and ds == 0.0:         # loss 0 and zero gradients by head_finalize_kernel and xscale
            assert not dz.any() and not dw.any() and not db.any()
            continue
        if case.storage == "bf16":
            assert dz.dtype == torch.bfloat16
            _stored_ok(dz.reshape(n, hw, c).cpu(), exp[0].cpu(), flips=5e-3)
            gz = 0.0
        else:
            gz = rel_err(dz.reshape(n, hw, c), exp[0])
        gw, gb = rel_err(dw, exp[1]), rel_err(db, exp[2])
        print(case.id, "bwd", (xs, ds, sc), "dz {:.2e} dw {:.2e} db {:.2e}".format(gz, gw, gb))
        assert gz < tol["grad"] and gw < tol["grad"] and gb < tol["grad"]


@pytest.mark.parametrize("mode", ["none", "numerical", "proportion"])
def test_restatement_agrees_with_oracle_losses(mode):
    """oracle.losses computes its weights in float32: a cross-check of the restatement, not the yardstick."""
    case = _case("x", 3, 480, 64, 3, mode, None)
    z, w, b, labels, _ = make_inputs(case)
    ref = ref_of(case, (z, w, b, labels, None), device="cpu")
    kw = {"numeric_w": numeric_w(3)} if mode == "numerical" else ({"proportion_decay": DECAY} if mode == "proportion" else {})
    lg = ref["logits"]
    xent = olosses.weighted_sparse_softmax_cross_entropy(lg.float(), labels.long(), mode, **kw).item()
    dice = olosses.sparse_dice_loss(torch.softmax(lg, -1), labels.long()).item()
    assert abs(xent - ref["xent"]) < 1e-6 * max(1.0, abs(ref["xent"]))
    assert abs(dice - ref["dice"]) < 1e-6


# ------------------------------------------------------------------------------------------------ refusals, inference, NaN
def _raw_buffers(d, c, storage_dtype=torch.float32):
    n, hw, ncls = d.N, d.HW, d.ncls
    g = torch.Generator().manual_seed(c)
    z = torch.randn((n * hw, c), generator=g).to(storage_dtype).cuda()
    w = (torch.randn((c, ncls), generator=g) * 0.3).cuda()
    b = (torch.randn(ncls, generator=g) * 0.1).cuda()
    labels = torch.randint(0, ncls, (n, hw), generator=g, dtype=torch.int32).cuda()
    nres = lib().unetk_head_result_floats(ctypes.byref(d))
    nws = lib().unetk_head_ws_bytes(ctypes.byref(d))
    assert nres > 0 and nws > 0
    return z, w, b, labels, nres, nws


@pytest.mark.parametrize("c", [6, 12, 20, 512])
def test_head_refuses_unsupported_widths_before_writing(ops, c):
    from boxsegliver_amd import _abi
    n, hw, ncls = 2, 40, 3
    d = ops.head_desc(n, hw, c, ncls)
    d.storage = _abi.FP32
    z, w, b, labels, nres, nws = _raw_buffers(d, c)
    sent = -12345.0
    logits = torch.full((n * hw, ncls), sent, device="cuda")
    probs, result = torch.full_like(logits, sent), torch.full((nres,), sent, device="cuda")
    ws = torch.full((nws // 4,), sent, device="cuda")
    rc = lib().unetk_head_fwd(ctypes.byref(d), _p(z), _p(w), _p(b), _p(labels), None, _p(logits), _p(probs), _p(result), _p(ws),
                              nws, _stream())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    for t in (logits, probs, result, ws):
        assert bool((t == sent).all())
    dz, dw, db = torch.full_like(z, sent), torch.full_like(w, sent), torch.full_like(b, sent)
    rc = lib().unetk_head_bwd(ctypes.byref(d), _p(z), _p(w), _p(labels), None, _p(logits), _p(result), 1.0, 1.0, None, _p(dz),
                              _p(dw), _p(db), _p(ws), nws, _stream())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    for t in (dz, dw, db, ws):
        assert bool((t == sent).all())
    with pytest.raises(_abi.UnetkError, match=r"\(code -2\)"):
        ops.head_fwd(d, z, w, b, labels)
    with pytest.raises(_abi.UnetkError, match=r"\(code -2\)"):
        ops.head_bwd(d, z, w, labels, None, logits, result, ws.view(torch.uint8), 1.0, 0.0)


@pytest.mark.parametrize("c,ncls,hw", [(64, 3, 1025), (32, 2, 255), (8, 8, 3)])
def test_head_inference_call_matches_labelled_and_leaves_result(ops, c, ncls, hw):
    from boxsegliver_amd import _abi
    n = 2
    d = ops.head_desc(n, hw, c, ncls)
    d.storage = _abi.FP32
    z, w, b, labels, nres, nws = _raw_buffers(d, c)
    lg, probs, _, _ = ops.head_fwd(d, z, w, b, labels, None, want_probs=True)
    lg2, probs2 = torch.full_like(lg, float("nan")), torch.full_like(lg, float("nan"))
    result = torch.full((nres,), 123.0, device="cuda")
    ws = torch.empty((nws,), dtype=torch.uint8, device="cuda")
    rc = lib().unetk_head_fwd(ctypes.byref(d), _p(z), _p(w), _p(b), None, None, _p(lg2), _p(probs2), _p(result), _p(ws), nws,
                              _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(_bits(lg), _bits(lg2)) and torch.equal(_bits(probs), _bits(probs2))
    assert bool((result == 123.0).all())


NAN_CASES = [
    ("proportion_no_decay_class_missing", "proportion", "missing", True),
    ("proportion_no_decay_all_present", "proportion", "random", False),
    ("numerical_present_classes_weigh_zero", "numerical", "zero_weight_only", True),
    ("numerical_mixed", "numerical", "random", False),
    ("nan_logit_at_one_pixel", "none", "nan_pixel", True),            # everything in front of the head hands its NaN over as this
    ("nan_logit_at_one_pixel_weighted", "numerical", "nan_pixel", True),
]


@pytest.mark.parametrize("name,mode,kind,expect_nan", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_head_loss_is_nan_exactly_when_the_formulas_give_nan(ops, name, mode, kind, expect_nan):
    """Pins behaviour (nan_watch relies on a NaN loss, not a finite wrong one): 1 / 0 normalised by inf under `proportion` without
    decay on a sample that lacks a class, and 0 / 0 under `numerical` where every class present in a sample weighs 0."""
    n, hw, c, ncls = 2, 96, 64, 3
    g = torch.Generator().manual_seed(len(name))
    z = torch.randn((n, hw, c), generator=g)
    w = torch.randn((c, ncls), generator=g) * 0.3
    b = torch.randn(ncls, generator=g) * 0.1
    labels = torch.randint(0, ncls, (n, hw), generator=g, dtype=torch.int32)
    labels[:, :3] = torch.arange(3, dtype=torch.int32)               # every class present ...
    if kind == "missing":
        labels[1][labels[1] == 2] = 0                                # ... but class 2 in sample 1
    elif kind == "zero_weight_only":
        labels[1] = 2                                                # NUMERIC_W[2] == 0
    elif kind == "nan_pixel":
        z[1, 37, 5] = float("nan")                                   # one activation: the three logits of that pixel are NaN
        labels[1, 37] = 1                                            # a class of non-zero weight in both modes
    nw = numeric_w(ncls)
    ref = head_ref(z, w, b, labels, mode, nw, None, None, grads=False)
    assert math.isnan(ref["xent"]) == expect_nan
    d = ops.head_desc(n, hw, c, ncls, mode, numeric_w=nw if mode == "numerical" else None)
    _, _, result, _ = ops.head_fwd(d, z.reshape(n * hw, c).cuda(), w.cuda(), b.cuda(), labels.cuda())
    got = result[0].item()
    assert math.isnan(got) == math.isnan(ref["xent"]), (got, ref["xent"])
    if not expect_nan:
        assert abs(got - ref["xent"]) < 2e-5 * max(1.0, abs(ref["xent"]))


def test_head_predict_on_nan_probabilities_follows_the_formulas(ops):
    """unetk_head_predict on what the softmax of a NaN logit leaves (every class NaN) and on a NaN in class 0 alone: the masks are
    p > 0.5, false for NaN, and the argmax keeps index 0 -- no class beats a NaN by `>`, and np.argmax names the first NaN too.
    Evaluated in float64 with numpy; the finite pixels around keep their answers.
    Deliberately NOT specified: a NaN in class 1 or 2 alone beside a finite class 0.  The kernel's `>` scan (as the reference's
    tf.argmax) skips it and names the largest finite class, np.argmax names the NaN; a softmax never produces that pixel, and this
    test does not pin "what argmax gives in float64" for it."""
    import numpy as np
    ncls, npix = 3, 1000
    p = np.random.default_rng(11).random((npix, ncls)).astype(np.float32)
    p[5] = np.nan                                                    # softmax(NaN logit): all classes
    p[700, 0] = np.nan                                               # class 0 alone
    p[701] = [0.1, 0.7, 0.2]
    amax, preds = ops.head_predict(torch.from_numpy(p).cuda(), ncls)
    p64 = p.astype(np.float64)
    with np.errstate(invalid="ignore"):
        want_preds = (p64[:, 1:] > 0.5).T.astype(np.uint8)
    want_amax = np.argmax(p64, -1).astype(np.uint8)
    assert want_amax[5] == 0 and want_amax[700] == 0 and want_amax[701] == 1 and not want_preds[:, 5].any()
    np.testing.assert_array_equal(amax.cpu().numpy(), want_amax)
    np.testing.assert_array_equal(preds.cpu().numpy(), want_preds)
