"""Host-side operators of the U-Net hot path: thin wrappers over the libunetk C ABI plus the
torch.autograd.Function nodes the networks are composed from.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); every FLOP and every
byte moved on the hot path happens inside a hand-written HIP kernel reached through
boxsegliver_amd._abi.  Nothing in this module falls back to torch ops or to the CPU oracle.

Reference call sites replaced (relative to the reference repo root):
  Conv3x3BnRelu : slim.repeat(x, 2, slim.conv2d, C, 3) unit           NetworksV2/UNet.py:79,85,94
  MaxPool2x2    : slim.max_pool2d(x, [2, 2])                           NetworksV2/UNet.py:81
  DeconvConcat  : slim.conv2d_transpose(x, C/2, 2, 2) + tf.concat      NetworksV2/UNet.py:91-93
  HeadLoss      : logits 1x1 conv + loss + metrics                     UNet.py:97-155, loss_metrics.py:115-339
"""
import ctypes
import os

import torch

from . import _abi
from ._abi import Conv3dDesc, ConvDesc, Deconv3dDesc, DeconvDesc, HeadDesc, NormDesc, check, ptr, stream_ptr


# ----------------------------------------------------------------------------- memory helpers
class _Workspace(object):
    """One growing scratch buffer per device; ops on one stream use it back to back."""

    def __init__(self):
        self._bufs = {}

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 16)
        key = (device.type, device.index)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf


WORKSPACE = _Workspace()
FUSE_EVAL = os.environ.get("UNETK_FUSE_EVAL", "1") != "0"    # inference: conv + (scale, shift) + ReLU [+ pool] in one kernel (0: two passes, measurement)
FUSE_NBR = True         # conv2's input gradient also emits conv1's norm-backward reduction (unetk_conv3x3_dgrad_nbr)
FUSED_NBR = {}          # dx.data_ptr() -> (producer y.data_ptr(), shape, partials, rows, dx._version); consumed by the producer's backward
DEBUG_CAPTURE = None    # tools/: set to a list to record each conv unit's backward operands
PROFILE_SHAPES = False  # bench.py --detail: one row per (kernel, layer shape)
PROFILE = None          # bench.py (profile_on): a list -> (op tag, algorithmic FLOPs, first trace record, end record, algorithmic bytes)


# ----------------------------------------------------------------------------- packed-filter cache
PACK_BATCH = True       # re-pack every known filter in ONE launch (unetk_pack_many) after the variables changed
PARAM_GEN = 0           # bumped by the kernels that write variables behind torch's back (optimiser steps, broadcasts)
_PARAM_FLATS = {}       # storage data_ptr of a ParamStore's flat buffer -> weakref to that tensor


def register_param_buffer(flat):
    """ParamStore: filters that are views of `flat` may keep their packed forms between steps."""
    import weakref
    _PARAM_FLATS[flat.untyped_storage().data_ptr()] = weakref.ref(flat)


def bump_param_gen():
    global PARAM_GEN
    PARAM_GEN += 1


class _PackItem(ctypes.Structure):            # unetk_pack_item
    _fields_ = [("kind", ctypes.c_int32), ("perm", ctypes.c_int32), ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32),
                ("block0", ctypes.c_int32), ("nblocks", ctypes.c_int32), ("r0", ctypes.c_int32), ("r1", ctypes.c_int32),
                ("w", ctypes.c_void_p), ("wp_fwd", ctypes.c_void_p), ("wp_dgrad", ctypes.c_void_p), ("r2", ctypes.c_void_p)]


class _PackCache(object):
    """Packed filters of the variables, kept between calls and rebuilt together.  An entry is valid while neither torch
    (the flat buffer's version counter) nor the optimiser kernels (PARAM_GEN) have written the variables since it was
    packed.  Only views of a registered ParamStore buffer are cached; anything else is packed on the spot."""

    def __init__(self):
        self.entries = {}          # key -> dict(flat=weakref, gen, wp_f, wp_d, items=[(kind, perm, cin, cout, w_ptr, f_ptr, d_ptr)])
        self.table = None          # (device tensor, n_items, total_blocks) of ALL live entries
        self.hits = self.batched = self.singles = 0

    @staticmethod
    def _flat_of(w):
        ref = _PARAM_FLATS.get(w.untyped_storage().data_ptr())
        return ref() if ref is not None else None

    def get(self, w, key, build):
        """build() -> (wp_f, wp_d, items): packs this filter alone.  Returns (wp_f, wp_d)."""
        flat = self._flat_of(w) if PACK_BATCH else None
        if flat is None:
            wp_f, wp_d, _ = build()
            return wp_f, wp_d
        key = (w.data_ptr(), tuple(w.shape)) + tuple(key)
        gen = (PARAM_GEN, flat._version)
        ent = self.entries.get(key)
        if ent is not None and ent["flat"]() is flat:
            if ent["gen"] == gen:
                self.hits += 1
                return ent["wp_f"], ent["wp_d"]
            self._repack_all()
            if ent["gen"] == gen:
                return ent["wp_f"], ent["wp_d"]
        import weakref
        for k in [k for k, e in self.entries.items() if e["flat"]() is None]:      # variables of models that are gone
            del self.entries[k]
            self.table = None
        wp_f, wp_d, items = build()
        self.singles += 1
        self.entries[key] = dict(flat=weakref.ref(flat), gen=gen, wp_f=wp_f, wp_d=wp_d, items=items)
        self.table = None
        return wp_f, wp_d

    def _repack_all(self):
        # strong references for the duration of the call: a collection cycle in the middle of it (a freed model's flat buffer)
        # must not turn a weak reference dead between this check and its use below
        held = {k: e["flat"]() for k, e in self.entries.items()}
        dead = [k for k, f in held.items() if f is None]
        for k in dead:
            del self.entries[k]
            self.table = None
        live = list(self.entries.values())
        if not live:
            return
        dev = live[0]["wp_f"].device
        if self.table is None:
            rows, block0 = [], 0
            for e in live:
                for kind, perm, cin, cout, w_ptr, f_ptr, d_ptr in e["items"]:
                    nb = _abi.lib().unetk_pack_item_blocks(kind, cin, cout)
                    if nb <= 0:
                        check(nb, "pack_item_blocks")
                    rows.append(_PackItem(kind, perm, cin, cout, block0, nb, 0, 0, w_ptr, f_ptr, d_ptr, None))
                    block0 += nb
            arr = (_PackItem * len(rows))(*rows)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self.table = (host.to(dev), len(rows), block0)
        tab, n_items, total = self.table
        check(_abi.lib().unetk_pack_many(ptr(tab), n_items, total, stream_ptr()), "pack_many")
        self.batched += 1
        for k, e in self.entries.items():
            e["gen"] = (PARAM_GEN, held[k]._version)


PACKS = _PackCache()
PK_CONV_F32, PK_CONV_BF16, PK_DECONV_F32, PK_DECONV_BF16 = 0, 1, 2, 3


class _Timed(object):
    """Brackets one C-ABI call with two marks of the library's kernel trace (csrc/prof.hip): while bench.py has the trace on,
    every kernel the call launches carries start / stop events bound to its dispatch, and the bracket is the half-open range of
    trace records [i0, i1) -- its time is the sum of those kernels' own GPU durations (what rocprofv3 --kernel-trace reports),
    with no host gap inside whatever the stream's queue depth was."""

    def __init__(self, tag, flops, shape=None, nbytes=0, by_kernel=False):
        """flops: algorithmic FLOPs of a matrix kernel; nbytes: algorithmic HBM bytes (each operand once) of an HBM-bound pass,
        or a function of the final tag.  by_kernel: the library picks the kernel (csrc/conv_igemm.hip, unetk_conv_plan), so the
        tag becomes the name of the first launch inside the bracket, read from the trace when the bracket closes; `tag` is
        kept only by a bracket that launched nothing."""
        self.on = PROFILE is not None
        self.tag, self.flops, self.shape, self.nbytes, self.by_kernel = tag, flops, shape, nbytes, by_kernel

    def __enter__(self):
        if self.on:
            self.i0 = _abi.lib().unetk_prof_mark()
        return self

    def __exit__(self, *exc):
        if self.on and exc[0] is None:
            i1 = _abi.lib().unetk_prof_mark()
            tag = _kernel_tag(self.i0) if self.by_kernel and i1 > self.i0 else self.tag
            nbytes = self.nbytes(tag) if callable(self.nbytes) else self.nbytes
            if PROFILE_SHAPES and self.shape:
                tag = "{} [{}]".format(tag, self.shape)
            PROFILE.append((tag, self.flops, self.i0, i1, nbytes))
        return False


def _kernel_tag(i):
    """Name of traced launch i as the tests and bench.py's tables write it: no "void ", no anonymous namespace, no argument
    list, no blanks -- conv3x3_igemm_kernel<2,2,4,2,1,1,0>."""
    buf = ctypes.create_string_buffer(512)
    check(_abi.lib().unetk_prof_name(i, buf, 512), "prof_name")
    return buf.value.decode().replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].replace(" ", "")


def profile_begin(reserve_launches=0):
    """bench.py: forget the kernel trace and pre-create its events (host work that must not sit in a timed region)."""
    check(_abi.lib().unetk_prof_reset(int(reserve_launches)), "prof_reset")


def profile_on(records):
    """Trace every launch of the library from here on and collect the op brackets into `records` (a list); None = off."""
    global PROFILE
    PROFILE = records
    check(_abi.lib().unetk_prof_enable(1 if records is not None else 0), "prof_enable")


def profile_read():
    """After a synchronize: (durations in ms, kernel names) of every traced launch since profile_begin()."""
    lib = _abi.lib()
    n = lib.unetk_prof_mark()
    ms = (ctypes.c_float * max(n, 1))()
    if n:
        check(lib.unetk_prof_read(0, n, ms), "prof_read")
    names, buf = [], ctypes.create_string_buffer(512)
    for i in range(n):
        check(lib.unetk_prof_name(i, buf, 512), "prof_name")
        names.append(buf.value.decode())
    return list(ms)[:n], names


class _NoTimer(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_TIMER = _NoTimer()


def _timed(tag_fn, flops, fmt=None, args=(), nbytes_fn=None, by_kernel=False):
    """Timer of a matrix kernel; tag_fn / the shape string / nbytes_fn are evaluated only when bench.py asked for events."""
    if PROFILE is None:
        return _NO_TIMER
    tag = tag_fn() if callable(tag_fn) else tag_fn
    return _Timed(tag, flops, fmt.format(*args) if fmt else None, nbytes_fn or 0, by_kernel)


def _timed_hbm(tag, t, passes, extra=0):
    """Timer of an HBM-bound pass moving `passes` x the bytes of tensor `t` (+ extra); a shared no-op unless bench.py asked
    for these (the byte count is not even computed then: these wrappers sit on the host path of every step)."""
    if PROFILE is None:
        return _NO_TIMER
    return _Timed(tag, 0.0, None, t.numel() * t.element_size() * passes + extra)


def alias(t, offset_elems=0, size=None, stride=None):
    """A fresh tensor object over t's storage (own autograd version counter).  The kernels write
    disjoint channel slices of shared concat buffers; autograd must not see those as in-place ops."""
    size = tuple(t.shape) if size is None else tuple(size)
    stride = tuple(t.stride()) if stride is None else tuple(stride)
    out = torch.empty(0, dtype=t.dtype, device=t.device)
    out.set_(t.untyped_storage(), t.storage_offset() + offset_elems, size, stride)
    return out


# ----------------------------------------------------------------------------- filter gradients on a second HIP stream
class _Side(object):
    """The filter gradient of a conv unit hangs off backward's critical chain (norm backward -> input gradient -> the
    previous unit's norm backward ...): nothing downstream reads dW before the optimiser.  With UNETK_SIDE_WGRAD=1 it is
    launched on a second HIP stream, ordered behind the main stream's dy, so the HBM-bound passes of the chain (norm
    backward, pool backward) can share the chip with it.  The main stream waits for the side stream at the end of the
    backward pass (autograd engine callback) and before a data-parallel bucket is all-reduced; dy and x are handed to the
    caching allocator as in use on the side stream (record_stream); the side stream has its own scratch buffer."""
    # Round 5: with the filter gradient queued BEFORE the unit's input gradient (SIDE_WGRAD_FIRST: the side stream then waits for
    # dy only and the two kernels really share the chip) the fp32 headline step gains 1.6 % in a same-call A/B (75.40 / 75.24 ->
    # 74.16 ms: the ~1.3 ms launches' tails fill each other), GUNet bs 8 nothing (21.44 vs 21.33-21.46), bf16 storage loses
    # (13.33 / 13.28 -> 13.42: its kernels hold all of a CU's LDS).  Default: on for fp32 units, off for the bf16 modes;
    # UNETK_SIDE_WGRAD=0 / 1 forces it off / on everywhere.
    mode = os.environ.get("UNETK_SIDE_WGRAD", "auto")
    enabled = mode != "0"
    paused = False          # bench.py: traced steps run on one stream (per-kernel durations that add up to the step)
    stream = None
    pending = False
    ws = _Workspace()


def side_wgrad_on(prec):
    """Does a 2-D conv unit of precision `prec` run its filter gradient on the side stream?"""
    if not _Side.enabled or _Side.paused:
        return False
    return _Side.mode == "1" or precision_of(prec) == _abi.FP32


def side_streams_pause(paused):
    """bench.py: pause (True) / resume (False) every use of the side stream (2-D and 3-D filter gradients)."""
    _Side.paused = bool(paused)


def side_join():
    """Order the current stream behind everything queued on the side stream (no-op when nothing is pending)."""
    if _Side.pending:
        torch.cuda.current_stream().wait_stream(_Side.stream)
        _Side.pending = False


# Tests only (tests/stream_delay.py): called as SIDE_LAUNCH_HOOK(kind, side) on the side stream, after its wait for the main
# stream and before the side work is queued; kind is "conv2d", "conv3d" or "deconv".  None: nothing is called.
SIDE_LAUNCH_HOOK = None


def _on_side(fn, keep, kind):
    """Queue fn() on the side stream, ordered behind what the current stream holds now.  `keep`: the tensors fn reads or
    scribbles on, handed to the caching allocator as in use on the side stream.  Every piece of side-stream work goes through
    here (tests/test_stream_order_host.py); the main stream joins in side_join()."""
    if _Side.stream is None:
        _Side.stream = torch.cuda.Stream(device=keep[0].device)
    side = _Side.stream
    side.wait_stream(torch.cuda.current_stream())          # the operands have been queued on the main stream
    with torch.cuda.stream(side):
        if SIDE_LAUNCH_HOOK is not None:
            SIDE_LAUNCH_HOOK(kind, side)
        out = fn()
    for t in keep:
        t.record_stream(side)
    if not _Side.pending:
        _Side.pending = True
        torch.autograd.Variable._execution_engine.queue_callback(side_join)
    return out


def _wgrad_on_side(x, dy, bf16, dilation, out):
    return _on_side(lambda: conv3x3_wgrad(x, dy, bf16=bf16, dilation=dilation, out=out, ws_pool=_Side.ws), (dy, x), "conv2d")


# 3-D layers: the filter gradient runs on the side stream BESIDE the input gradient.  UNet3D at one or two patches per GPU is a
# sequence of 100-800 us launches of a few hundred tiles whose tails leave CUs idle (and the bridge's 27-54 blocks never fill the
# chip); two such launches side by side share it.  Same kernels, same results bit for bit.  Measured in one call, 96^3: 20.52 ->
# 20.29 ms at one patch, 38.0 -> 37.6 at two (the bridge alone: no gain; 10 x 256 x 256: no change).  Threshold in output
# voxels of the layer (0 = never); UNETK_SIDE_WGRAD3D overrides.
# Round 5 (the advisor's finding): round 4 queued the side-stream launch AFTER the input gradient, so the side stream's
# wait_stream(main) made the filter gradient wait for that input gradient too -- it ran beside the NEXT unit's norm backward, not
# beside "its" input gradient as the text above says.  *_FIRST (default): it is queued BEFORE the input gradient, behind dy only.
# Same-call A/Bs: UNet3D 96^3 at one patch 20.51 -> 19.97 ms, at two 37.83 -> 36.93; the fp32 2-D headline 75.3 -> 74.2 ms.
SIDE_WGRAD3D_VOXELS = int(os.environ.get("UNETK_SIDE_WGRAD3D", str(1 << 20)))
SIDE_WGRAD_FIRST = os.environ.get("UNETK_SIDE_WGRAD_FIRST", "1") == "1"          # the 2-D units (see _Side)
SIDE_WGRAD3D_FIRST = os.environ.get("UNETK_SIDE_WGRAD3D_FIRST", "1") == "1"      # the 3-D units (Conv3dNormRelu.backward)


def _wgrad3d_on_side(x, dy, d, out, precision=0):
    return _on_side(lambda: conv3d_wgrad(x, dy, d, out=out, ws_pool=_Side.ws, precision=precision), (dy, x), "conv3d")


# ----------------------------------------------------------------------------- in-place parameter gradients
class _GradSink(object):
    """Parameter gradients written by the backward kernels straight into the variable's slice of the flat gradient
    buffer (ParamStore.grad) instead of a fresh tensor that autograd then adds to it: 65 tiny add launches per step
    gone.  A slot is written in place at most once between two new_step() calls (ParamStore.zero_grad), and only when
    the variable has exactly ONE recorded use (`uses`, counted by the forwards that end up on an autograd tape; the count
    restarts with the first recorded forward after a backward -- Solver.__call__ runs zero_grad BETWEEN the forward and
    its backward, so zero_grad cannot be the reset point): a variable shared by two ops takes the returned-tensor path
    for every use, i.e. autograd sums the contributions and the post-accumulate hook fires once, after the sum -- the
    data-parallel buckets must never see an arrival that precedes the variable's last contribution.  A denied slot is
    always safe (autograd accumulates).  `hooks` maps a slot to the callback the buckets would have got from a
    post-accumulate hook."""
    written = set()
    uses = {}
    tape = True         # is the forward being run recorded on an autograd tape (set by _Op.apply)
    stale = False       # a backward has run since `uses` was last cleared: the next recorded forward starts a fresh count
    hooks = {}
    enabled = True


class _Op(torch.autograd.Function):
    """Base of the libunetk autograd nodes: notes, before the forward runs (inside it grad mode is always off and
    needs_input_grad is set regardless), whether a tape is recording -- an evaluation forward under torch.no_grad() must
    not count as a use of its parameters (grad_sink)."""

    @classmethod
    def apply(cls, *args, **kwargs):
        # saved and restored: an op applied INSIDE another op's forward (the SE gate's FullyConnected under
        # torch.enable_grad()) must not leave its own answer behind for the outer forward's grad_sink() calls
        prev = _GradSink.tape
        _GradSink.tape = torch.is_grad_enabled()
        try:
            return super(_Op, cls).apply(*args, **kwargs)
        finally:
            _GradSink.tape = prev


def new_step(bufs=None):
    """Start of a step for the gradient buffers `bufs` (a ParamStore's flat gradient tensors; None = every slot): their
    slots may be written in place again.  Another model's slots keep their state (its own zero_grad resets them)."""
    if bufs is None:
        _GradSink.written.clear()
    else:
        spans = [(b.data_ptr(), b.data_ptr() + b.numel() * b.element_size()) for b in bufs]
        _GradSink.written.difference_update([k for k in _GradSink.written if any(lo <= k < hi for lo, hi in spans)])
    FUSED_NBR.clear()
    if _Side.pending:           # a backward that raised left filter gradients on the side stream un-joined
        side_join()


def grad_sink(p, ctx=None):
    """The flat-gradient slot of leaf parameter `p` when a backward kernel may write it in place, else None.  Called from
    an op's forward with its autograd context: a forward no tape records (torch.no_grad(): evaluation) is not a use."""
    if not _GradSink.enabled or p is None or not p.is_leaf or not p.requires_grad:
        return None
    if ctx is not None and not _GradSink.tape:
        return None
    g = p.grad
    if g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.shape != p.shape:
        return None
    if _GradSink.stale:
        _GradSink.uses.clear()
        _GradSink.stale = False
    k = g.data_ptr()
    _GradSink.uses[k] = _GradSink.uses.get(k, 0) + 1
    return g


def _take(slot):
    """Claim `slot` for an in-place write in this step (None if absent, already written, or used more than once)."""
    _GradSink.stale = True
    if slot is None:
        return None
    k = slot.data_ptr()
    if k in _GradSink.written or _GradSink.uses.get(k, 0) != 1:
        return None
    _GradSink.written.add(k)
    return slot


def _ret(value, slot):
    """What a backward returns for a parameter: None when its gradient already sits in `slot` (the bucket hook fires
    here, after the kernel was queued), else the tensor for autograd to accumulate."""
    if slot is None:
        return value
    hook = _GradSink.hooks.get(slot.data_ptr())
    if hook is not None:
        hook()
    return None


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _abi.UnetkError("libunetk ops need device tensors (got a CPU tensor); "
                                  "there is no CPU path in the product")


def _pix_stride(t):
    """Pixel stride (floats) of an NHWC tensor whose channel dim is contiguous."""
    assert t.dim() == 4 and t.stride(3) == 1, "NHWC with contiguous channels expected"
    s = t.stride(2)
    assert t.stride(1) == t.shape[2] * s and t.stride(0) == t.shape[1] * t.shape[2] * s, \
        "only a channel-slice view of a dense NHWC buffer is supported"
    return s


# ----------------------------------------------------------------------------- raw op wrappers
def conv_uses_bf16(cin, cout):
    """UNETK_BF16 kernels exist for Cin % 32 == 0 and Cout % 32 == 0; other layers (the first conv) stay fp32."""
    return cin % 32 == 0 and cout % 32 == 0


def precision_of(flag):
    """NormSpec.bf16 / --compute_dtype -> UNETK_FP32 (0) | UNETK_BF16 (1: bf16 MFMA operands, fp32 tensors) |
    UNETK_BF16S (2: bf16 MFMA + bf16 STORAGE of activations and activation gradients, include/unetk.h)."""
    if flag is True:
        return _abi.BF16
    return int(flag or 0)


def storage_dtype(prec):
    return torch.bfloat16 if int(prec) == _abi.BF16S else torch.float32


def _storage_of(t):
    """Descriptor `storage` value of an activation tensor."""
    if t.dtype == torch.bfloat16:
        return _abi.BF16S
    assert t.dtype == torch.float32, t.dtype
    return _abi.FP32


def conv3x3_pack(w, want_dgrad=True, bf16=False):
    _require_cuda(w)
    kh, kw, cin, cout = w.shape
    assert kh == 3 and kw == 3
    prec = precision_of(bf16)

    def build():
        if prec:
            wp_f = torch.empty(9 * cin * cout, dtype=torch.bfloat16, device=w.device)
            wp_d = torch.empty_like(wp_f) if want_dgrad else None
            if prec == _abi.BF16S:          # output channels pair-permuted inside 64-blocks (conv_igemm_bf16.hip)
                check(_abi.lib().unetk_conv3x3_pack_bf16s(ptr(w), cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()),
                      "conv3x3_pack_bf16s")
            else:
                check(_abi.lib().unetk_conv3x3_pack_bf16(ptr(w), cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()),
                      "conv3x3_pack_bf16")
            kind, perm = PK_CONV_BF16, 1 if prec == _abi.BF16S else 0
        else:
            wp_f = torch.empty(9 * cin * cout, dtype=torch.float32, device=w.device)
            wp_d = torch.empty_like(wp_f) if want_dgrad else None
            check(_abi.lib().unetk_conv3x3_pack(ptr(w), cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()), "conv3x3_pack")
            kind, perm = PK_CONV_F32, 0
        return wp_f, wp_d, [(kind, perm, cin, cout, w.data_ptr(), wp_f.data_ptr(), wp_d.data_ptr() if want_dgrad else None)]
    return PACKS.get(w, ("c3", prec, bool(want_dgrad)), build)


def conv_uses_mfma(cin, cout):
    return cin % 16 == 0 and cout % 32 == 0


def conv3x3_fwd(x, w, cout, want_stats=True, y=None, bf16=False, dilation=1):
    """x NHWC (pixel-strided ok); w = packed filter if conv_uses_mfma(cin, cout) else raw HWIO.
    bf16 = precision (precision_of): under UNETK_BF16S x is bf16 (fp32 for the direct first-layer kernel) and y is bf16."""
    _require_cuda(x, w)
    n, h, wd, cin = x.shape
    prec = precision_of(bf16)
    if y is None:
        y = torch.empty((n, h, wd, cout), dtype=storage_dtype(prec), device=x.device)
    if prec == _abi.BF16S:
        assert y.dtype == torch.bfloat16 and x.dtype == (torch.bfloat16 if conv_uses_mfma(cin, cout) else torch.float32), \
            (x.dtype, y.dtype, cin, cout)
    else:
        assert x.dtype == torch.float32 and y.dtype == torch.float32
    d = ConvDesc(n, h, wd, cin, cout, _pix_stride(x), _pix_stride(y), prec, int(dilation))
    stats = None
    rows = 0
    if want_stats:
        rows = _abi.lib().unetk_conv3x3_stat_rows(ctypes.byref(d))
        if rows <= 0:
            check(rows, "conv3x3_stat_rows")
        stats = torch.empty((2, rows, cout), dtype=torch.float32, device=x.device)
    nws = _abi.lib().unetk_conv3x3_ws_bytes(ctypes.byref(d)) if prec == _abi.FP32 else 0     # stream-K scratch (small planes)
    ws = WORKSPACE.get(nws, x.device) if nws else None
    # the first layer's direct kernel is HBM-bound (writes 64 channels per pixel from 3): reported by bytes as well
    with _timed("conv3x3_fwd", 18.0 * n * h * wd * cin * cout, "fwd {}x{}x{} {}->{}", (n, h, wd, cin, cout),
                lambda tag: (x.numel() * x.element_size() + y.numel() * y.element_size()) if tag.startswith(("conv3x3_direct_kernel", "conv3x3_c3_mfma_kernel")) else 0,
                by_kernel=True):
        check(_abi.lib().unetk_conv3x3_fwd_ws(ctypes.byref(d), ptr(x), ptr(w), ptr(y), ptr(stats), ptr(ws), nws,
                                              stream_ptr()), "conv3x3_fwd")
    return y, stats, rows


def conv3x3_fwd_affine(x, w, cout, scale, shift, z=None, pool=False, bf16=False):
    """Inference: z = relu(conv3x3(x, w) * scale + shift) [and max_pool2d(z, 2, 2)] in one kernel (unetk_conv3x3_fwd_affine);
    w as for conv3x3_fwd.  Returns (z, pooled or None); raises UNETK_E_UNSUPPORTED shapes (ask conv3x3_fwd_affine_ok first)."""
    _require_cuda(x, w)
    n, h, wd, cin = x.shape
    prec = precision_of(bf16)
    if z is None:
        z = torch.empty((n, h, wd, cout), dtype=storage_dtype(prec), device=x.device)
    d = ConvDesc(n, h, wd, cin, cout, _pix_stride(x), _pix_stride(z), prec, 1)
    pooled = torch.empty((n, h // 2, wd // 2, cout), dtype=z.dtype, device=x.device) if pool else None
    nws = _abi.lib().unetk_conv3x3_ws_bytes(ctypes.byref(d))
    ws = WORKSPACE.get(nws, x.device) if nws else None
    check(_abi.lib().unetk_conv3x3_fwd_affine(ctypes.byref(d), ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(z), ptr(pooled), cout,
                                              ptr(ws), nws, stream_ptr()), "conv3x3_fwd_affine")
    return z, pooled


def conv3x3_fwd_affine_ok(n, h, wd, cin, cout, pool=False, bf16=False):
    d = ConvDesc(n, h, wd, cin, cout, cin, cout, precision_of(bf16), 1)
    return _abi.lib().unetk_conv3x3_fwd_affine_ok(ctypes.byref(d), 1 if pool else 0) == 1


def conv3x3_dgrad(dy, wp_dgrad, cin, x_stride=None, dx=None, bf16=False, dilation=1, producer=None):
    """producer = (y, aff, per_sample) of the unit whose activation is this conv's input: the kernel then also emits that
    unit's norm-backward reduction (unetk_conv3x3_dgrad_nbr) and the partials are left in FUSED_NBR for its backward."""
    _require_cuda(dy, wp_dgrad)
    n, h, wd, cout = dy.shape
    prec = precision_of(bf16)
    assert dy.dtype == storage_dtype(prec), (dy.dtype, prec)
    if dx is None:
        dx = torch.empty((n, h, wd, cin), dtype=dy.dtype, device=dy.device)
    d = ConvDesc(n, h, wd, cin, cout, _pix_stride(dx), _pix_stride(dy), prec, int(dilation))
    if producer is not None and FUSE_NBR:
        py, paff, per_sample = producer
        rows = _abi.lib().unetk_conv3x3_dgrad_nbr_rows(ctypes.byref(d))
        if rows > 0 and py.dtype == dx.dtype and tuple(py.shape) == tuple(dx.shape) and py.is_contiguous():
            part = torch.empty((2, rows, cin), dtype=torch.float32, device=dy.device)
            with _timed("conv3x3_dgrad_nbr", 18.0 * n * h * wd * cin * cout, "dgrad+nbr {}x{}x{} {}->{}", (n, h, wd, cout, cin),
                        by_kernel=True):
                check(_abi.lib().unetk_conv3x3_dgrad_nbr(ctypes.byref(d), ptr(dy), ptr(wp_dgrad), ptr(dx), ptr(py), cin,
                                                         ptr(paff[2]), ptr(paff[3]), ptr(paff[0]), ptr(paff[1]),
                                                         1 if per_sample else 0, ptr(part), stream_ptr()),
                      "conv3x3_dgrad_nbr")
            # dx._version: when the producer's activation has a SECOND consumer, autograd sums the gradients IN PLACE into
            # this tensor (same data_ptr, same shape) -- the partials computed from this dx alone would be stale; any in-place
            # accumulation bumps the version counter, and the producer's backward then ignores the entry
            FUSED_NBR[dx.data_ptr()] = (py.data_ptr(), tuple(dx.shape), part, rows, dx._version)
            return dx
    nws = _abi.lib().unetk_conv3x3_ws_bytes(ctypes.byref(d)) if prec == _abi.FP32 else 0
    ws = WORKSPACE.get(nws, dy.device) if nws else None
    with _timed("conv3x3_dgrad", 18.0 * n * h * wd * cin * cout, "dgrad {}x{}x{} {}->{}", (n, h, wd, cout, cin), by_kernel=True):
        check(_abi.lib().unetk_conv3x3_dgrad_ws(ctypes.byref(d), ptr(dy), ptr(wp_dgrad), ptr(dx), ptr(ws), nws, stream_ptr()),
              "conv3x3_dgrad")
    return dx


def conv3x3_wgrad(x, dy, bf16=False, dilation=1, out=None, ws_pool=None):
    _require_cuda(x, dy)
    n, h, wd, cin = x.shape
    cout = dy.shape[3]
    prec = precision_of(bf16)
    if prec == _abi.BF16S:
        assert dy.dtype == torch.bfloat16 and x.dtype == (torch.bfloat16 if cin % 64 == 0 else torch.float32), (x.dtype, dy.dtype)
    d = ConvDesc(n, h, wd, cin, cout, _pix_stride(x), _pix_stride(dy), prec, int(dilation))
    nbytes = _abi.lib().unetk_conv3x3_wgrad_ws_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise _abi.UnetkError("conv3x3_wgrad: unsupported shape Cin={} Cout={}".format(cin, cout))
    ws = (ws_pool or WORKSPACE).get(nbytes, x.device)
    dw = out if out is not None else torch.empty((3, 3, cin, cout), dtype=torch.float32, device=x.device)
    assert tuple(dw.shape) == (3, 3, cin, cout) and dw.is_contiguous()
    tag = "conv3x3_wgrad_kernel(+slab_reduce)" if cin % 64 == 0 else "conv3x3_wgrad_c3_kernel(+slab_reduce)"
    if bf16 and cin % 32 == 0:
        tag = "conv3x3_wgrad_kernel<bf16>(+slab_reduce)"
    if prec == _abi.BF16S:
        tag = "conv3x3_wgrad_bf16s_kernel(+slab_reduce)" if cin % 64 == 0 else "conv3x3_wgrad_c3_bf16s_kernel(+slab_reduce)"
    with _timed(tag, 18.0 * n * h * wd * cin * cout, "{}x{}x{} {}->{}", (n, h, wd, cin, cout)):
        check(_abi.lib().unetk_conv3x3_wgrad(ctypes.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(ws), nbytes,
                                             stream_ptr()), "conv3x3_wgrad")
    return dw


def conv3d_desc(x_shape, cout, kd, stride, x_stride=None, y_stride=None, live8=None):
    """live8 = (cin mask, cout mask) of a channel-padded filter (NetworksV2/padded.py live8_masks): bit i = channels
    [8 i, 8 i + 8) hold a real channel; the kernels skip the dead groups of their contraction axis (include/unetk.h)."""
    n, dd, h, w, cin = x_shape
    sd, sh, sw = stride
    assert sh == sw, "H and W strides must match"
    d = Conv3dDesc(n, dd, h, w, cin, cout, kd, sd, sh, x_stride or cin, y_stride or cout)
    if live8 is not None:
        for field, m in ((d.cin_live8, live8[0]), (d.cout_live8, live8[1])):
            field[0], field[1] = m & 0xFFFFFFFF, (m >> 32) & 0xFFFFFFFF
    return d


def conv3d_out_shape(d):
    do, ho, wo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_abi.lib().unetk_conv3d_out_dims(ctypes.byref(d), ctypes.byref(do), ctypes.byref(ho), ctypes.byref(wo)),
          "conv3d_out_dims")
    return (d.N, do.value, ho.value, wo.value, d.Cout)


def conv3d_bf16_ok(d):
    """The UNETK_BF16 layer rule of the 3-D convs (include/unetk.h): stride 1, Cin % 32 == 0, Cout % 32 == 0, kd in {1, 3}."""
    return d.sd == 1 and d.shw == 1 and d.kd in (1, 3) and d.Cin % 32 == 0 and d.Cout % 32 == 0


def conv3d_precision(d, precision):
    """The precision a 3-D conv of descriptor d runs at when the net asks for `precision`: UNETK_BF16 only for the layers the
    rule admits, every other layer stays exact fp32 (the caller need not know which)."""
    return _abi.BF16 if int(precision or 0) == _abi.BF16 and conv3d_bf16_ok(d) else _abi.FP32


def conv3d_pack(w, want_dgrad=True, precision=0):
    """w: TF DHWIO [kd,3,3,Cin,Cout] (Cin % 4 == 0 for the MFMA path).  precision UNETK_BF16: kd bf16 K8 packs (one per
    depth tap, the layout of unetk_conv3x3_pack_bf16), Cin % 32 == 0 and Cout % 32 == 0."""
    _require_cuda(w)
    kd, kh, kw, cin, cout = w.shape
    assert kh == 3 and kw == 3
    prec = int(precision or 0)
    if prec not in (_abi.FP32, _abi.BF16):
        raise _abi.UnetkError("conv3d_pack: precision {} is not built for the 3-D convs".format(prec))
    if prec == _abi.BF16:
        def build_bf16():
            wp_f = torch.empty(kd * 9 * cin * cout, dtype=torch.bfloat16, device=w.device)
            wp_d = torch.empty_like(wp_f) if want_dgrad else None
            check(_abi.lib().unetk_conv3d_pack_bf16(ptr(w), kd, cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()),
                  "conv3d_pack_bf16")
            src, tap = 9 * cin * cout * 4, 9 * cin * cout * 2        # bytes per depth tap: fp32 source, bf16 packs
            items = [(PK_CONV_BF16, 0, cin, cout, w.data_ptr() + a * src, wp_f.data_ptr() + a * tap,
                      (wp_d.data_ptr() + a * tap) if want_dgrad else None) for a in range(kd)]
            return wp_f, wp_d, items
        return PACKS.get(w, ("c3d", prec, bool(want_dgrad)), build_bf16)

    def build():
        wp_f = torch.empty(kd * 9 * cin * cout, dtype=torch.float32, device=w.device)
        wp_d = torch.empty_like(wp_f) if want_dgrad else None
        check(_abi.lib().unetk_conv3d_pack(ptr(w), kd, cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()), "conv3d_pack")
        tap = 9 * cin * cout * 4            # bytes per depth tap, source and packs alike
        items = [(PK_CONV_F32, 0, cin, cout, w.data_ptr() + a * tap, wp_f.data_ptr() + a * tap,
                  (wp_d.data_ptr() + a * tap) if want_dgrad else None) for a in range(kd)]
        return wp_f, wp_d, items
    return PACKS.get(w, ("c3d", 0, bool(want_dgrad)), build)


def _bf16_3d(d, precision):
    """True when the call runs the UNETK_BF16 entry points; a bf16 request for a layer outside the rule is an error here
    (Conv3dNormRelu picks the layer's precision with conv3d_precision)."""
    if int(precision or 0) == _abi.FP32:
        return False
    if int(precision) != _abi.BF16 or not conv3d_bf16_ok(d):
        raise _abi.UnetkError("conv3d: precision {} is not built for kd={} stride=({},{}) Cin={} Cout={}".format(
            int(precision), d.kd, d.sd, d.shw, d.Cin, d.Cout))
    return True


def _ws3d(d, device, bf16=False, pool=None):
    nbytes = (_abi.lib().unetk_conv3d_ws_bytes_bf16 if bf16 else _abi.lib().unetk_conv3d_ws_bytes)(ctypes.byref(d))
    return (pool or WORKSPACE).get(nbytes, device), nbytes


def conv3d_fwd(x, w, d, want_stats=True, precision=0):
    """x [N,D,H,W,Cin] dense; w = packed filter when conv_uses_mfma(Cin, Cout) else raw DHWIO (kd == 1).
    precision UNETK_BF16: bf16 matrix-core operands (w from conv3d_pack(..., precision=UNETK_BF16)), fp32 tensors."""
    _require_cuda(x, w)
    assert x.stride(-1) == 1 and x.stride(-2) == d.x_stride        # dense, or a channel slice of a concat buffer
    bf16 = _bf16_3d(d, precision)
    y = torch.empty(conv3d_out_shape(d), dtype=torch.float32, device=x.device)
    stats, rows = None, 0
    if want_stats:
        rows = (_abi.lib().unetk_conv3d_stat_rows_bf16 if bf16 else _abi.lib().unetk_conv3d_stat_rows)(ctypes.byref(d))
        if rows <= 0:
            check(rows, "conv3d_stat_rows")
        stats = torch.empty((2, rows, d.Cout), dtype=torch.float32, device=x.device)
    ws, nbytes = _ws3d(d, x.device, bf16)
    flops = 2.0 * y.numel() / d.Cout * d.kd * 9 * d.Cin * d.Cout
    fn = _abi.lib().unetk_conv3d_fwd_bf16 if bf16 else _abi.lib().unetk_conv3d_fwd
    with _Timed("conv3d_fwd<bf16>" if bf16 else "conv3d_fwd", flops, "k{}s{}{} {}".format(d.kd, d.sd, d.shw, tuple(x.shape))):
        check(fn(ctypes.byref(d), ptr(x), ptr(w), ptr(y), ptr(stats), ptr(ws), nbytes, stream_ptr()), "conv3d_fwd")
    return y, stats, rows


def conv3d_dgrad(dy, wp_dgrad, d, precision=0):
    assert dy.is_contiguous()
    bf16 = _bf16_3d(d, precision)
    dx = torch.empty((d.N, d.D, d.H, d.W, d.Cin), dtype=torch.float32, device=dy.device)
    ws, nbytes = _ws3d(d, dy.device, bf16)
    flops = 2.0 * dy.numel() / d.Cout * d.kd * 9 * d.Cin * d.Cout
    fn = _abi.lib().unetk_conv3d_dgrad_bf16 if bf16 else _abi.lib().unetk_conv3d_dgrad
    with _Timed("conv3d_dgrad<bf16>" if bf16 else "conv3d_dgrad", flops, "k{}s{}{} {}".format(d.kd, d.sd, d.shw, tuple(dx.shape))):
        check(fn(ctypes.byref(d), ptr(dy), ptr(wp_dgrad), ptr(dx), ptr(ws), nbytes, stream_ptr()), "conv3d_dgrad")
    return dx


def conv3d_wgrad(x, dy, d, out=None, ws_pool=None, precision=0):
    assert x.stride(-2) == d.x_stride and dy.is_contiguous()
    bf16 = _bf16_3d(d, precision)
    dw = out if out is not None else torch.empty((d.kd, 3, 3, d.Cin, d.Cout), dtype=torch.float32, device=x.device)
    assert tuple(dw.shape) == (d.kd, 3, 3, d.Cin, d.Cout) and dw.is_contiguous()
    ws, nbytes = _ws3d(d, x.device, bf16, ws_pool)
    flops = 2.0 * dy.numel() / d.Cout * d.kd * 9 * d.Cin * d.Cout
    fn = _abi.lib().unetk_conv3d_wgrad_bf16 if bf16 else _abi.lib().unetk_conv3d_wgrad
    with _Timed("conv3d_wgrad<bf16>" if bf16 else "conv3d_wgrad", flops, "k{}s{}{} {}".format(d.kd, d.sd, d.shw, tuple(x.shape))):
        check(fn(ctypes.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(ws), nbytes, stream_ptr()), "conv3d_wgrad")
    return dw


def norm_desc(y_shape, per_sample, z_stride=None, guide_ch=0, gw_stride=0, gw_coff=0):
    n, c = y_shape[0], y_shape[-1]
    hw = 1
    for s in y_shape[1:-1]:
        hw *= s
    return NormDesc(n, hw, c, 1 if per_sample else 0, z_stride if z_stride is not None else c, guide_ch,
                    gw_stride, gw_coff)


def norm_finalize(d, stats, rows, gamma, beta, eps, decay, training, moving_mean, moving_var, device, y=None):
    """y: the fp32 activations the partials were taken of; given, the ill-conditioned channels (mean^2 > 16 (var + eps))
    get their statistics from a second, shifted pass over y (unetk_norm_finalize_y).  bf16 storage passes none."""
    groups = d.N if d.per_sample else 1
    out = torch.empty((4, groups, d.C), dtype=torch.float32, device=device)   # mean, rstd, scale, shift
    nbytes = _abi.lib().unetk_norm_finalize_ws_bytes(ctypes.byref(d), max(rows, groups))
    ws = WORKSPACE.get(nbytes, device)
    if y is not None:
        if y.dtype != torch.float32:
            y = None
        else:
            assert y.is_contiguous() and y.numel() == d.N * d.HW * d.C, (tuple(y.shape), d.N, d.HW, d.C)
    check(_abi.lib().unetk_norm_finalize_y(ctypes.byref(d), ptr(stats), rows, ptr(y), ptr(gamma), ptr(beta), eps, decay,
                                           1 if training else 0, ptr(moving_mean), ptr(moving_var), ptr(out[0]),
                                           ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(ws), nbytes, stream_ptr()),
          "norm_finalize")
    return out


def norm_apply_relu(d, y, aff, z, guide=None, gw=None, gb=None, den=None):
    assert y.is_contiguous() and y.dtype == z.dtype
    d.storage = _storage_of(y)
    if den is not None:
        assert den.is_contiguous() and tuple(den.shape) == (d.N, d.C), (tuple(den.shape), d.N, d.C)
    with _timed_hbm("norm_apply_relu", y, 2):          # read y, write z
        check(_abi.lib().unetk_norm_apply_relu(ctypes.byref(d), ptr(y), ptr(aff[2]), ptr(aff[3]), ptr(den), ptr(guide),
                                               ptr(gw), ptr(gb), ptr(z), stream_ptr()), "norm_apply_relu")
    return z


def _norm_refused(op, d):
    """unetk_norm_bwd_ws_bytes(d) == 0: the backward refuses the descriptor whatever operands come with it (NormPlan, norm.hip)."""
    return ("{}: the norm descriptor is refused (N {} HW {} C {} guide_ch {} guide_leaky {} storage {} dropout_keep {}): the backward "
            "needs N, HW > 0, C % 4 == 0, C <= 1024, guide_ch in 0..4, fp32 or bf16 storage, dropout_keep in [0, 1] and a guide "
            "under guide_leaky").format(op, d.N, d.HW, d.C, d.guide_ch, d.guide_leaky, d.storage, d.dropout_keep)


def norm_relu_bwd(d, y, dz, aff, has_gamma, has_beta, guide=None, gw=None, gb=None, den=None, out_gamma=None,
                  out_beta=None, pre=None):
    dev = y.device
    assert dz.dtype == y.dtype, (dz.dtype, y.dtype)
    d.storage = _storage_of(y)
    dy = torch.empty_like(y)
    dden = torch.empty_like(den) if den is not None else None
    dgamma = (out_gamma if out_gamma is not None else torch.empty((d.C,), dtype=torch.float32, device=dev)) if has_gamma else None
    dbeta = (out_beta if out_beta is not None else torch.empty((d.C,), dtype=torch.float32, device=dev)) if has_beta else None
    blk = (4,) if d.guide_leaky == 3 else ()       # guide_leaky == 3: gb is the block [bias, slope+, slope-, post-shift] and so is its gradient
    if d.guide_per_sample:
        dgw = torch.empty((d.N, d.guide_ch, d.C), dtype=torch.float32, device=dev) if d.guide_ch else None
        dgb = torch.empty((d.N,) + blk + (d.C,), dtype=torch.float32, device=dev) if (d.guide_ch or gb is not None) else None
    else:
        dgw = torch.empty((d.guide_ch, d.C), dtype=torch.float32, device=dev) if d.guide_ch else None
        dgb = torch.empty(blk + (d.C,), dtype=torch.float32, device=dev) if (d.guide_ch or gb is not None) else None
    nbytes = _abi.lib().unetk_norm_bwd_ws_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise _abi.UnetkError(_norm_refused("norm_relu_bwd", d))
    ws = WORKSPACE.get(nbytes, dev)
    pre_part, pre_rows = pre if pre is not None else (None, 0)
    # reduction pass reads (dz, y) unless its partials came from the producing kernel; the apply pass reads (dz, y), writes dy
    with _timed_hbm("norm_relu_bwd(apply only)" if pre is not None else "norm_relu_bwd(reduce+apply)", y, 3 if pre is not None else 5):
        check(_abi.lib().unetk_norm_relu_bwd_pre(ctypes.byref(d), ptr(y), ptr(dz), _pix_stride_nd(dz), ptr(aff[2]), ptr(aff[3]),
                                                 ptr(aff[0]), ptr(aff[1]), ptr(den), ptr(guide), ptr(gw), ptr(gb), ptr(dy),
                                                 ptr(dgamma), ptr(dbeta), ptr(dden), ptr(dgw), ptr(dgb), ptr(pre_part),
                                                 int(pre_rows), ptr(ws), nbytes, stream_ptr()),
              "norm_relu_bwd")
    if den is not None:
        return dy, dgamma, dbeta, dgw, dgb, dden
    return dy, dgamma, dbeta, dgw, dgb


def norm_apply_relu_pool(d, y, aff, z):
    """z = relu(y * scale + shift) and max_pool2d(z, 2, 2) in one pass (unetk_norm_apply_relu_pool); returns the pooled tensor."""
    d.storage = _storage_of(y)
    n, h, w, c = y.shape
    pooled = torch.empty((n, h // 2, w // 2, c), dtype=y.dtype, device=y.device)
    with _timed_hbm("norm_apply_relu_pool", y, 2.25):
        check(_abi.lib().unetk_norm_apply_relu_pool(ctypes.byref(d), int(w), ptr(y), ptr(aff[2]), ptr(aff[3]), ptr(z), ptr(pooled),
                                                    stream_ptr()), "norm_apply_relu_pool")
    return pooled


def norm_relu_bwd_pool(d, y, dskip, dp, aff, has_gamma, has_beta, out_gamma=None, out_beta=None):
    """norm_relu_bwd of a plain unit whose activation feeds max_pool2d AND the skip connection, with the pool's backward
    folded in (unetk_norm_relu_bwd_pool): dz = dskip + route(dp) is never written.  y [N, H, W, C]."""
    dev = y.device
    assert dskip.dtype == y.dtype and dp.dtype == y.dtype and dp.is_contiguous()
    d.storage = _storage_of(y)
    dy = torch.empty_like(y)
    dgamma = (out_gamma if out_gamma is not None else torch.empty((d.C,), dtype=torch.float32, device=dev)) if has_gamma else None
    dbeta = (out_beta if out_beta is not None else torch.empty((d.C,), dtype=torch.float32, device=dev)) if has_beta else None
    nbytes = _abi.lib().unetk_norm_bwd_ws_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise _abi.UnetkError(_norm_refused("norm_relu_bwd_pool", d))
    ws = WORKSPACE.get(nbytes, dev)
    # both passes read (y, dskip) and a quarter-size dp; the apply pass writes dy
    with _timed_hbm("norm_relu_bwd_pool(reduce+apply)", y, 5.5):
        check(_abi.lib().unetk_norm_relu_bwd_pool(ctypes.byref(d), int(y.shape[2]), ptr(y), ptr(dskip), _pix_stride_nd(dskip),
                                                  ptr(dp), ptr(aff[2]), ptr(aff[3]), ptr(aff[0]), ptr(aff[1]), ptr(dy),
                                                  ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, stream_ptr()),
              "norm_relu_bwd_pool")
    return dy, dgamma, dbeta


norm_relu_bwd_nd = norm_relu_bwd     # rank-agnostic (dz pixel stride = stride of the second-to-last axis)


def sobel_concat(x, ch):
    """InterUNet --img_grad: concat(x, sobel_dy(x[..., ch]), sobel_dx(x[..., ch])) (InterUNet.py:105-109); no gradient."""
    _require_cuda(x)
    x = x.to(torch.float32).contiguous()
    n, h, w, c = x.shape
    out = torch.empty((n, h, w, c + 2), dtype=torch.float32, device=x.device)
    check(_abi.lib().unetk_sobel_concat(ptr(x), ptr(out), n, h, w, c, int(ch), stream_ptr()), "sobel_concat")
    return out


def image_gradients(x):
    """--img_grad: concat(x, dy, dx) along channels (UNet.py:69-71); the input needs no gradient."""
    _require_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty((n, h, w, 3 * c), dtype=torch.float32, device=x.device)
    check(_abi.lib().unetk_image_gradients(ptr(x.contiguous()), ptr(out), n, h, w, c, stream_ptr()), "image_gradients")
    return out


def flip_axpy(x, out=None, flip_h=False, flip_w=False, scale=1.0, accumulate=False):
    """out (+)= scale * flip(x) over H and/or W of an NHWC tensor (mirror TTA, evaluator_liver.py:648-655)."""
    _require_cuda(x)
    x = x.contiguous()
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty_like(x)
        accumulate = False
    assert out.is_contiguous() and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    check(_abi.lib().unetk_flip_axpy(ptr(x), ptr(out), n, h, w, c, int(bool(flip_h)), int(bool(flip_w)), float(scale),
                                     int(bool(accumulate)), stream_ptr()), "flip_axpy")
    return out


def avgpool2_fwd(x):
    _require_cuda(x)
    n, h, w, c = x.shape
    p = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    check(_abi.lib().unetk_avgpool2_fwd(ptr(x.contiguous()), ptr(p), n, h, w, c, stream_ptr()), "avgpool2_fwd")
    return p


def maxpool2_fwd(x):
    _require_cuda(x)
    n, h, w, c = x.shape
    p = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    fn = _abi.lib().unetk_maxpool2_fwd_bf16 if _storage_of(x) == _abi.BF16S else _abi.lib().unetk_maxpool2_fwd
    with _timed_hbm("maxpool2_fwd", p, 5):            # reads x (4 p), writes p
        check(fn(ptr(x), _pix_stride(x), ptr(p), n, h, w, c, stream_ptr()), "maxpool2_fwd")
    return p


def maxpool2_bwd(x, p, dp, add=None):
    """dx = route(dp) [+ add]; `add` may be a channel slice of a wider NHWC buffer (the concat buffer's gradient)."""
    n, h, w, c = x.shape
    dx = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device)
    assert dp.dtype == x.dtype and p.dtype == x.dtype
    if add is not None:
        assert tuple(add.shape) == (n, h, w, c) and add.stride(3) == 1 and add.dtype == x.dtype
    fn = _abi.lib().unetk_maxpool2_bwd_bf16 if _storage_of(x) == _abi.BF16S else _abi.lib().unetk_maxpool2_bwd
    # reads x, p, dp (+ the skip gradient), writes dx
    with _timed_hbm("maxpool2_bwd", p, (4 * 3 if add is not None else 4 * 2) + 2):
        check(fn(ptr(x), _pix_stride(x), ptr(p), ptr(dp.contiguous()), ptr(add),
                 _pix_stride(add) if add is not None else 0, ptr(dx), n, h, w, c, stream_ptr()), "maxpool2_bwd")
    return dx


def deconv2x2_pack(w, bf16=False):
    _require_cuda(w)
    kh, kw, cout, cin = w.shape
    assert kh == 2 and kw == 2
    prec = precision_of(bf16)

    def build():
        if prec:
            wp_f = torch.empty(4 * cin * cout, dtype=torch.bfloat16, device=w.device)
            wp_d = torch.empty_like(wp_f)
            if prec == _abi.BF16S:
                check(_abi.lib().unetk_deconv2x2_pack_bf16s(ptr(w), cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()),
                      "deconv2x2_pack_bf16s")
            else:
                check(_abi.lib().unetk_deconv2x2_pack_bf16(ptr(w), cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()),
                      "deconv2x2_pack_bf16")
            kind, perm = PK_DECONV_BF16, 1 if prec == _abi.BF16S else 0
        else:
            wp_f = torch.empty(4 * cin * cout, dtype=torch.float32, device=w.device)
            wp_d = torch.empty_like(wp_f)
            check(_abi.lib().unetk_deconv2x2_pack(ptr(w), cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()), "deconv2x2_pack")
            kind, perm = PK_DECONV_F32, 0
        return wp_f, wp_d, [(kind, perm, cin, cout, w.data_ptr(), wp_f.data_ptr(), wp_d.data_ptr())]
    return PACKS.get(w, ("d2", prec, True), build)


def deconv2x2_fwd(x, wp_fwd, bias, cat, coff, cout, bf16=False):
    n, h, w, cin = x.shape
    assert x.is_contiguous()
    prec = precision_of(bf16)
    assert x.dtype == storage_dtype(prec) and cat.dtype == x.dtype, (x.dtype, cat.dtype, prec)
    d = DeconvDesc(n, h, w, cin, cout, _pix_stride(cat), coff, prec)
    tag = {0: "pw_gemm_kernel<fwd>", 1: "pw_gemm_bf16_kernel<fwd>", 2: "pw_gemm_bf16_kernel<fwd,bs>"}[prec]
    with _timed(tag, 8.0 * n * h * w * cin * cout, "{}x{}x{} {}->{}", (n, h, w, cin, cout)):
        check(_abi.lib().unetk_deconv2x2_fwd(ctypes.byref(d), ptr(x), ptr(wp_fwd), ptr(bias), ptr(cat), stream_ptr()),
              "deconv2x2_fwd")
    return cat


# Round 5: the transposed conv's filter gradient on the side stream as well.  Its backward is ReLU mask -> input gradient -> filter
# gradient in one C call; only dx is on backward's critical chain.  unetk_deconv*_bwd_parts does the first two on the main stream
# and the filter gradient (which reads the masked gradient the first part left in the scratch buffer) on the side stream, beside
# the next unit's norm backward / input gradient.  The scratch buffer is then the op's own (the shared WORKSPACE is rewritten by
# the next op on the main stream).  Needs the in-place gradient slot (otherwise autograd would add dw on the main stream at once).
SIDE_DECONV = os.environ.get("UNETK_SIDE_DECONV", "1") == "1"


def _deconv_bwd_call(fn_parts, fn_whole, d, nbytes, args, side_ok, what):
    """args = (x, wp_dgrad, cat, dcat, dx, dw, db) pointers' owners; returns nothing (dx / dw / db are filled)."""
    xx, wp, cat, dcat, dx, dw, db = args
    if not (side_ok and SIDE_DECONV and not _Side.paused):
        ws = WORKSPACE.get(nbytes, xx.device)
        check(fn_whole(ctypes.byref(d), ptr(xx), ptr(wp), ptr(cat), ptr(dcat), ptr(dx), ptr(dw), ptr(db), ptr(ws), nbytes,
                       stream_ptr()), what)
        return
    ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=xx.device)
    check(fn_parts(ctypes.byref(d), ptr(xx), ptr(wp), ptr(cat), ptr(dcat), ptr(dx), ptr(dw), ptr(db), ptr(ws), nbytes, 1,
                   stream_ptr()), what)
    _on_side(lambda: check(fn_parts(ctypes.byref(d), ptr(xx), ptr(wp), ptr(cat), ptr(dcat), ptr(dx), ptr(dw), ptr(db), ptr(ws),
                                    nbytes, 2, stream_ptr()), what), (ws, xx), "deconv")


def deconv2x2_bwd(x, wp_dgrad, cat, dcat, coff, cout, bf16=False, out_w=None, out_b=None):
    n, h, w, cin = x.shape
    prec = precision_of(bf16)
    assert x.dtype == storage_dtype(prec) and cat.dtype == x.dtype and dcat.dtype == x.dtype
    d = DeconvDesc(n, h, w, cin, cout, _pix_stride(cat), coff, prec)
    assert _pix_stride(dcat) == _pix_stride(cat)
    nbytes = _abi.lib().unetk_deconv2x2_bwd_ws_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise _abi.UnetkError("deconv2x2_bwd: unsupported shape Cin={} Cout={}".format(cin, cout))
    dx = torch.empty_like(x)
    dw = out_w if out_w is not None else torch.empty((2, 2, cout, cin), dtype=torch.float32, device=x.device)
    db = out_b if out_b is not None else torch.empty((cout,), dtype=torch.float32, device=x.device)
    assert tuple(dw.shape) == (2, 2, cout, cin) and dw.is_contiguous()
    side_ok = out_w is not None and DEBUG_CAPTURE is None and side_wgrad_on(bf16)
    with _timed(lambda: "deconv2x2_bwd{}(relu_bwd+pw_gemm<dgrad>+deconv_wgrad)".format({0: "", 1: "<bf16>", 2: "<bf16s>"}[prec]),
                16.0 * n * h * w * cin * cout, "{}x{}x{} {}->{}", (n, h, w, cin, cout)):
        _deconv_bwd_call(_abi.lib().unetk_deconv2x2_bwd_parts, _abi.lib().unetk_deconv2x2_bwd, d, nbytes,
                         (x, wp_dgrad, cat, dcat, dx, dw, db), side_ok, "deconv2x2_bwd")
    return dx, dw, db


def deconv3d_pack(w, precision=0):
    """w: TF [kd,2,2,Cout,Cin] with kd in {1, 2}.  precision UNETK_BF16: the bf16 packs (Cin % 32 == 0 and Cout % 32 == 0)."""
    _require_cuda(w)
    kd, kh, kw, cout, cin = w.shape
    assert kh == 2 and kw == 2 and kd in (1, 2)
    prec = int(precision or 0)
    if prec not in (_abi.FP32, _abi.BF16):
        raise _abi.UnetkError("deconv3d_pack: precision {} is not built for the 3-D transposed convs".format(prec))
    if prec == _abi.BF16:
        def build_bf16():
            wp_f = torch.empty(kd * 4 * cin * cout, dtype=torch.bfloat16, device=w.device)
            wp_d = torch.empty_like(wp_f)
            check(_abi.lib().unetk_deconv3d_pack_bf16(ptr(w), kd, cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()),
                  "deconv3d_pack_bf16")
            src, tap = 4 * cin * cout * 4, 4 * cin * cout * 2
            items = [(PK_DECONV_BF16, 0, cin, cout, w.data_ptr() + a * src, wp_f.data_ptr() + a * tap,
                      wp_d.data_ptr() + a * tap) for a in range(kd)]
            return wp_f, wp_d, items
        return PACKS.get(w, ("d3d", prec, True), build_bf16)

    def build():
        wp_f = torch.empty(kd * 4 * cin * cout, dtype=torch.float32, device=w.device)
        wp_d = torch.empty_like(wp_f)
        check(_abi.lib().unetk_deconv3d_pack(ptr(w), kd, cin, cout, ptr(wp_f), ptr(wp_d), stream_ptr()), "deconv3d_pack")
        tap = 4 * cin * cout * 4
        items = [(PK_DECONV_F32, 0, cin, cout, w.data_ptr() + a * tap, wp_f.data_ptr() + a * tap, wp_d.data_ptr() + a * tap)
                 for a in range(kd)]
        return wp_f, wp_d, items
    return PACKS.get(w, ("d3d", 0, True), build)


def _pix_stride_nd(t):
    """Pixel stride of a channel-slice view of a dense N...C tensor."""
    assert t.stride(-1) == 1
    return t.stride(-2)


def deconv3d_fwd(x, wp_fwd, bias, cat, coff, cout, kd, precision=0):
    n, dd, h, w, cin = x.shape
    assert x.is_contiguous()
    d = Deconv3dDesc(n, dd, h, w, cin, cout, kd, _pix_stride_nd(cat), coff, int(precision or 0))
    with _Timed("deconv3d_fwd", 8.0 * kd * n * dd * h * w * cin * cout, "kd{} {}".format(kd, tuple(x.shape))):
        check(_abi.lib().unetk_deconv3d_fwd(ctypes.byref(d), ptr(x), ptr(wp_fwd), ptr(bias), ptr(cat), stream_ptr()),
              "deconv3d_fwd")
    return cat


def deconv3d_bwd(x, wp_dgrad, cat, dcat, coff, cout, kd, want_dbias, out_w=None, precision=0):
    n, dd, h, w, cin = x.shape
    d = Deconv3dDesc(n, dd, h, w, cin, cout, kd, _pix_stride_nd(cat), coff, int(precision or 0))
    assert _pix_stride_nd(dcat) == _pix_stride_nd(cat)
    nbytes = _abi.lib().unetk_deconv3d_bwd_ws_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise _abi.UnetkError("deconv3d_bwd: unsupported shape Cin={} Cout={}".format(cin, cout))
    dx = torch.empty_like(x)
    dw = out_w if out_w is not None else torch.empty((kd, 2, 2, cout, cin), dtype=torch.float32, device=x.device)
    assert tuple(dw.shape) == (kd, 2, 2, cout, cin) and dw.is_contiguous()
    db = torch.empty((cout,), dtype=torch.float32, device=x.device) if want_dbias else None
    side_ok = out_w is not None and DEBUG_CAPTURE is None and _Side.enabled and SIDE_WGRAD3D_VOXELS > 0
    with _Timed("deconv3d_bwd", 16.0 * kd * n * dd * h * w * cin * cout, "kd{} {}".format(kd, tuple(x.shape))):
        _deconv_bwd_call(_abi.lib().unetk_deconv3d_bwd_parts, _abi.lib().unetk_deconv3d_bwd, d, nbytes,
                         (x, wp_dgrad, cat, dcat, dx, dw, db), side_ok, "deconv3d_bwd")
    return dx, dw, db


def head_desc(n, hw, c, ncls, weight_mode="none", numeric_w=None, proportion_decay=0.0):
    mode = {"none": _abi.W_NONE, "numerical": _abi.W_NUMERICAL, "proportion": _abi.W_PROPORTION,
            "pixelmap": _abi.W_PIXELMAP}[weight_mode]
    d = HeadDesc()
    d.N, d.HW, d.C, d.ncls, d.weight_mode = n, hw, c, ncls, mode
    if mode == _abi.W_NUMERICAL:
        if numeric_w is None or len(numeric_w) != ncls:
            raise KeyError("w_type `numerical` need keyword argument `numeric_w`")
        for i, v in enumerate(numeric_w):
            d.numeric_w[i] = float(v)
    d.proportion_decay = float(proportion_decay or 0.0)
    return d


def head_fwd(d, z, w, b, labels, pixel_w=None, want_probs=False):
    _require_cuda(z, w, b)
    npix = d.N * d.HW
    dev = z.device
    assert z.is_contiguous()
    d.storage = _storage_of(z)
    logits = torch.empty((npix, d.ncls), dtype=torch.float32, device=dev)
    probs = torch.empty_like(logits) if want_probs else None
    nres = _abi.lib().unetk_head_result_floats(ctypes.byref(d))
    nbytes = _abi.lib().unetk_head_ws_bytes(ctypes.byref(d))
    if nres == 0 or nbytes == 0:
        raise _abi.UnetkError("head: bad descriptor")
    result = torch.zeros((nres,), dtype=torch.float32, device=dev)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)    # kept for backward (weight tables)
    with _timed_hbm("head_fwd", z, 1, npix * (4 + 4 * d.ncls * (2 if want_probs else 1))):
        check(_abi.lib().unetk_head_fwd(ctypes.byref(d), ptr(z), ptr(w), ptr(b), ptr(labels), ptr(pixel_w), ptr(logits),
                                        ptr(probs), ptr(result), ptr(ws), nbytes, stream_ptr()), "head_fwd")
    return logits, probs, result, ws


def head_bwd(d, z, w, labels, pixel_w, logits, result, ws, xent_scale, dice_scale, dev_scales=None, out_w=None, out_b=None):
    d.storage = _storage_of(z)
    dz = torch.empty_like(z)
    dw = out_w if out_w is not None else torch.empty((d.C, d.ncls), dtype=torch.float32, device=z.device)
    db = out_b if out_b is not None else torch.empty((d.ncls,), dtype=torch.float32, device=z.device)
    assert tuple(dw.shape) == (d.C, d.ncls) and dw.is_contiguous()
    with _timed_hbm("head_bwd", z, 2, d.N * d.HW * (4 + 4 * d.ncls)):
        check(_abi.lib().unetk_head_bwd(ctypes.byref(d), ptr(z), ptr(w), ptr(labels), ptr(pixel_w), ptr(logits), ptr(result),
                                        float(xent_scale), float(dice_scale), ptr(dev_scales), ptr(dz), ptr(dw), ptr(db),
                                        ptr(ws), ws.numel(), stream_ptr()), "head_bwd")
    return dz, dw, db


def head_predict(probs, ncls, want_preds=True):
    npix = probs.numel() // ncls
    amax = torch.empty((npix,), dtype=torch.uint8, device=probs.device)
    preds = torch.empty((ncls - 1, npix), dtype=torch.uint8, device=probs.device) if want_preds else None
    check(_abi.lib().unetk_head_predict(ptr(probs), npix, ncls, ptr(amax), ptr(preds), stream_ptr()), "head_predict")
    return amax, preds


def boundary_weights(labels):
    """--loss_weight_type boundary (loss_metrics.py:149-165): labels int32 [N,H,W] -> normalised weight map f32."""
    _require_cuda(labels)
    if labels.dim() != 3:
        raise ValueError("loss_weight_type `boundary` is defined for [bs, H, W] labels only (loss_metrics.py:150-151)")
    labels = labels.to(torch.int32).contiguous()
    n, h, w = labels.shape
    wmap = torch.empty((n, h, w), dtype=torch.float32, device=labels.device)
    nbytes = _abi.lib().unetk_boundary_weights_ws_bytes(n, h, w)
    ws = WORKSPACE.get(nbytes, labels.device)
    check(_abi.lib().unetk_boundary_weights(ptr(labels), n, h, w, ptr(wmap), ptr(ws), nbytes, stream_ptr()),
          "boundary_weights")
    return wmap


def boundary_weights3d(labels, z_scale=1, want_d2=False):
    """--loss_weight_type boundary for UNet3D: labels int32 [N,D,H,W] -> normalised weight map f32
    [N,D,H,W]; z_scale = the slice spacing in units of the in-plane spacing (an integer, 1..16).  want_d2: also the exact
    squared distances int32 [N,D,H,W] (-1 throughout a sample without a ring voxel, whose weights are all 1)."""
    _require_cuda(labels)
    if labels.dim() != 4:
        raise ValueError("boundary_weights3d takes [bs, D, H, W] labels, got shape {}".format(tuple(labels.shape)))
    labels = labels.to(torch.int32).contiguous()
    n, d, h, w = labels.shape
    wmap = torch.empty((n, d, h, w), dtype=torch.float32, device=labels.device)
    d2 = torch.empty((n, d, h, w), dtype=torch.int32, device=labels.device) if want_d2 else None
    nbytes = _abi.lib().unetk_boundary_weights3d_ws_bytes(n, d, h, w)
    ws = WORKSPACE.get(nbytes, labels.device)
    check(_abi.lib().unetk_boundary_weights3d(ptr(labels), n, d, h, w, int(z_scale), ptr(wmap), ptr(d2), ptr(ws), nbytes,
                                              stream_ptr()), "boundary_weights3d")
    return (wmap, d2) if want_d2 else wmap


# ----------------------------------------------------------------------------- volume evaluation (csrc/evalvol.hip)
def _mask3d(t):
    """A [D, H, W] device mask as a dense uint8 tensor (non-zero = object)."""
    _require_cuda(t)
    if t.dim() != 3:
        raise ValueError("a 3-D [D, H, W] mask expected, got shape {}".format(tuple(t.shape)))
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = t != 0
        t = t.view(torch.uint8)
    return t.contiguous()


def largest_component3d(mask):
    """utils/array_kits.get_largest_component(mask, rank=3) on the device: the largest 6-connected component as a 0/1
    uint8 mask, zeros for an empty mask.  One device-to-host read (the size of the largest component and how many share
    it).  When several share it, the host's rule -- the last index of np.argsort(areas) over the components in scipy's
    label order, which np.argsort's unstable sort decides for long arrays -- is applied to the component sizes the
    kernel left in its workspace, exactly as the host computes it."""
    import numpy as np
    m = _mask3d(mask)
    d, h, w = m.shape
    n = d * h * w
    out = torch.empty_like(m)
    info = torch.empty(4, dtype=torch.int32, device=m.device)
    lib = _abi.lib()
    nbytes = lib.unetk_largest_component_ws_bytes(d, h, w)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=m.device)
    check(lib.unetk_largest_component(ptr(m), d, h, w, ptr(out), ptr(info), ptr(ws), nbytes, stream_ptr()),
          "largest_component3d")
    _, _, ties, _ = info.tolist()
    if ties > 1:
        off = (4 * n + 255) & ~255
        sizes = ws[off:off + 4 * n].view(torch.int32)
        roots = torch.nonzero(sizes).flatten()                     # ascending = scipy's label order
        areas = sizes[roots].cpu().numpy().astype(np.int64)
        root = int(roots[int(np.argsort(areas)[-1])])
        check(lib.unetk_component_mask(ptr(ws), d, h, w, root, ptr(out), stream_ptr()), "component_mask")
    return out


def fp_mask3d(pred, lab, pred_label, obj_label, min_size=6, out_value=64, lab_scale=64):
    """The false-positive objects of a predicted volume (unetk_fp_mask3d; include/unetk.h has the rule): pred, lab uint8
    [D, H, W] on the device, lab in the store's encoding.  Returns (out uint8 [D, H, W] = out_value on the 6-connected
    components of pred >= pred_label with >= min_size voxels and no voxel on lab / lab_scale >= obj_label, slice_counts int32
    [D], head int32 [4] = {components, kept components, kept voxels, 0}), all on the device.  Current stream."""
    _require_cuda(pred, lab)
    assert pred.dtype == torch.uint8 and pred.dim() == 3 and pred.is_contiguous()
    assert lab.dtype == torch.uint8 and lab.shape == pred.shape and lab.is_contiguous()
    d, h, w = pred.shape
    lib = _abi.lib()
    nbytes = int(lib.unetk_fp_mask3d_ws_bytes(d, h, w))
    if nbytes == 0:
        raise _abi.UnetkError("fp_mask3d: a volume of {} x {} x {} voxels is not supported".format(d, h, w))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    out = torch.empty_like(pred)
    counts = torch.empty(d, dtype=torch.int32, device=pred.device)
    head = torch.empty(4, dtype=torch.int32, device=pred.device)
    check(lib.unetk_fp_mask3d(ptr(pred), ptr(lab), d, h, w, int(pred_label), int(lab_scale), int(obj_label), int(min_size),
                              int(out_value), ptr(out), ptr(counts), ptr(head), ptr(ws), nbytes, stream_ptr()), "fp_mask3d")
    return out, counts, head


def component_overlaps_table(res, ref, cap_obj=65536, cap_pair=262144, table=None, ws=None):
    """unetk_component_overlaps as the kernel leaves it: the int32 device table [4 + 4 cap_obj + 3 cap_pair] (include/unetk.h)
    of the 6-connected components of two same-shape masks and of the pairs that share voxels.  No host read."""
    res, ref = _mask3d(res), _mask3d(ref)
    if res.shape != ref.shape:
        raise ValueError("shape mismatch: {} and {}".format(tuple(res.shape), tuple(ref.shape)))
    d, h, w = res.shape
    cap_obj, cap_pair = int(cap_obj), int(cap_pair)
    lib = _abi.lib()
    nbytes = lib.unetk_component_overlaps_ws_bytes(d, h, w, cap_obj, cap_pair)
    if nbytes == 0:
        raise ValueError("unsupported component_overlaps shape {} / caps {} {}".format(tuple(res.shape), cap_obj, cap_pair))
    if table is None:
        table = torch.empty(4 + 4 * cap_obj + 3 * cap_pair, dtype=torch.int32, device=res.device)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=res.device)
    check(lib.unetk_component_overlaps(ptr(res), ptr(ref), d, h, w, cap_obj, cap_pair, ptr(table), ptr(ws), ws.numel(),
                                       stream_ptr()), "component_overlaps")
    return table


def component_overlaps(res, ref, cap_obj=65536, cap_pair=262144):
    """The component tables of per-lesion detection (utils/array_kits.distinct_binary_object_correspondences) from the
    device: (res_sizes int64 [n_res], ref_sizes int64 [n_ref], pairs int64 [n_pair, 3] rows (ref_id, res_id, overlap) sorted
    by (ref_id, res_id)) as numpy arrays, ids 1-based in scipy.ndimage.label's order with 6-connectivity.  One
    device-to-host read of the table.  Raises RuntimeError naming the cap that is too small; never a truncated table."""
    import numpy as np
    cap_obj, cap_pair = int(cap_obj), int(cap_pair)
    table = component_overlaps_table(res, ref, cap_obj, cap_pair).cpu().numpy()
    n_res, n_ref, n_pair, overflow = (int(v) for v in table[:4])
    if overflow:
        over = []
        if overflow & 1:
            over.append("cap_obj = {} < {} result components".format(cap_obj, n_res))
        if overflow & 2:
            over.append("cap_obj = {} < {} reference components".format(cap_obj, n_ref))
        if overflow & 4:
            over.append("cap_pair = {} < {} overlapping pairs".format(cap_pair, n_pair))
        raise RuntimeError("component_overlaps: " + "; ".join(over))
    rows = table[4:4 + 4 * cap_obj].reshape(2, cap_obj, 2)
    pairs = table[4 + 4 * cap_obj:].reshape(cap_pair, 3)[:n_pair]
    return rows[0, :n_res, 1].astype(np.int64), rows[1, :n_ref, 1].astype(np.int64), pairs.astype(np.int64)


_HIST_TABLES = {}


def hist_bin_table(bins=100, xrng=(-200, 250)):
    """The host side of unetk_slice_hist for integer HU values: (lut int32 [n], lut_lo, db float64 [bins]).  lut[v - lut_lo]
    is the bin np.histogram(v, bins, range=xrng) puts the integer v in (asked of numpy itself, value by value, so its edge
    rule and closed last bin hold exactly), -1 where it counts nothing; db = np.diff of its float64 edges."""
    import math
    import numpy as np
    key = (int(bins), float(xrng[0]), float(xrng[1]))
    if key not in _HIST_TABLES:
        lo, hi = int(math.ceil(key[1])), int(math.floor(key[2]))
        if hi < lo:
            raise ValueError("the range {} holds no integer value".format(xrng))
        lut = np.full(hi - lo + 1, -1, dtype=np.int32)
        for v in range(lo, hi + 1):
            h, edges = np.histogram(np.array([v], dtype=np.int16), bins=key[0], range=key[1:])
            if h.any():
                lut[v - lo] = int(np.argmax(h))
        _HIST_TABLES[key] = (lut, lo, np.diff(edges).astype(np.float64))
    return _HIST_TABLES[key]


def slice_hist(vol, lab, mode, bins=100, xrng=(-200, 250)):
    """float32 [D, 2 bins] per-slice density histograms of a case (unetk_slice_hist): vol int16 [D, H, W] HU, lab uint8
    [D, H, W] on the device; mode "train" (second half: lab == 2 of the slice) or "eval" (second half: the middle slices of
    the 18-connected tumours covering the slice) -- extract.py dump_hist_feature / dump_hist_feature_v2, bit for bit."""
    import numpy as np
    _require_cuda(vol, lab)
    if mode not in ("train", "eval"):
        raise ValueError("mode must be `train` or `eval`, got {}".format(mode))
    if vol.dtype != torch.int16 or lab.dtype != torch.uint8 or vol.dim() != 3 or vol.shape != lab.shape:
        raise ValueError("int16 volume and uint8 labels of one [D, H, W] shape expected, got {} {} and {} {}".format(
            vol.dtype, tuple(vol.shape), lab.dtype, tuple(lab.shape)))
    vol, lab = vol.contiguous(), lab.contiguous()
    d, h, w = vol.shape
    lut, lut_lo, db = hist_bin_table(bins, xrng)
    tabs = torch.from_numpy(np.concatenate([db.view(np.int32), lut])).to(vol.device)     # one upload: db (8-aligned), lut
    m = 0 if mode == "train" else 1
    out = torch.empty((d, 2 * bins), dtype=torch.float32, device=vol.device)
    lib = _abi.lib()
    nbytes = lib.unetk_slice_hist_ws_bytes(d, h, w, int(bins), m)
    if nbytes == 0:
        raise ValueError("unsupported slice_hist shape {} / bins {}".format(tuple(vol.shape), bins))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    check(lib.unetk_slice_hist(ptr(vol), ptr(lab), d, h, w, m, ptr(tabs[2 * bins:]), lut_lo, len(lut), ptr(tabs), int(bins),
                               ptr(out), ptr(ws), nbytes, stream_ptr()), "slice_hist")
    return out


GLCM_PROPERTIES = ("contrast", "dissimilarity", "homogeneity", "energy", "entropy", "correlation", "cluster_shade",
                   "cluster_prominence")


def glcm_offsets(distances=(1, 2, 3), angles=(0, 1, 2, 3)):
    """int32 [len(distances) * len(angles), 2] = (dr, dc) of skimage's greycomatrix for the angles a * pi / 4:
    (round(sin(a pi / 4) d), round(cos(a pi / 4) d)), in the order distance-major, the reference's [d][a] layout."""
    import math
    import numpy as np
    return np.array([[int(round(math.sin(a * math.pi / 4) * d)), int(round(math.cos(a * math.pi / 4) * d))]
                     for d in distances for a in angles], dtype=np.int32).reshape(-1, 2)


def glcm_features(patches, offsets=None, norm_levels=True, want_counts=False, device=None):
    """float64 numpy [n, 8 K] texture features of n uint8 patches (unetk_glcm_features; include/unetk.h has the definition):
    column = property * K + offset index, the reference's np.array([ff[fe] for fe in feat_list]).reshape(-1) with
    K = distances x angles.  patches: 2-D uint8 numpy arrays of any sizes up to 4096 x 4096; they are packed back to back
    into one pinned buffer and uploaded in one copy.  offsets: int [K, 2] (default glcm_offsets()).  want_counts: also the
    uint32 [n, K, 256, 256] symmetric count matrices."""
    import numpy as np
    offs = np.ascontiguousarray(glcm_offsets() if offsets is None else offsets, dtype=np.int32).reshape(-1, 2)
    n, k = len(patches), offs.shape[0]
    device = device or torch.device("cuda", torch.cuda.current_device())
    tab = np.zeros((max(n, 1), 3), dtype=np.int32)
    total = 0
    for i, a in enumerate(patches):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("patch {}: a 2-D uint8 numpy array expected".format(i))
        tab[i] = (total, a.shape[0], a.shape[1])
        total += a.size
    lib = _abi.lib()
    nbytes = int(lib.unetk_glcm_features_ws_bytes(n, k))
    if nbytes == 0 or total >= 1 << 31:
        raise _abi.UnetkError("glcm_features: unsupported request ({} patches, {} offsets, {} bytes)".format(n, k, total))
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for a, (o, _, _) in zip(patches, tab):
        hv[o:o + a.size] = a.reshape(-1)
    pix = host.to(device, non_blocking=True)
    out = torch.empty((n, 8, k), dtype=torch.float64, device=device)
    counts = torch.empty((n, k, 256, 256), dtype=torch.int32, device=device) if want_counts else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.unetk_glcm_features(ptr(pix), total, tab.ctypes.data_as(ctypes.c_void_p), n,
                                      offs.ctypes.data_as(ctypes.c_void_p), k, 1 if norm_levels else 0, ptr(out), ptr(counts),
                                      ptr(ws), nbytes, stream_ptr()), "glcm_features")
        feats = out.cpu().numpy().reshape(n, 8 * k)          # also ends the library's read of the host table
    if want_counts:
        return feats, counts.cpu().numpy().view(np.uint32)
    return feats


def mask_counts_async(a, b):
    """int64 device tensor {|A|, |B|, |A and B|, |A or B|} of two same-shape masks (no host read)."""
    a, b = _mask3d(a), _mask3d(b)
    if a.shape != b.shape:
        raise ValueError("shape mismatch: {} and {}".format(tuple(a.shape), tuple(b.shape)))
    d, h, w = a.shape
    counts = torch.empty(4, dtype=torch.int64, device=a.device)
    nbytes = _abi.lib().unetk_mask_counts_ws_bytes(d, h, w)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)
    check(_abi.lib().unetk_mask_counts(ptr(a), ptr(b), d, h, w, ptr(counts), ptr(ws), nbytes, stream_ptr()), "mask_counts")
    return counts


def mask_counts(a, b):
    """Confusion counts of a test mask `a` against a reference mask `b` (loss_metrics.ConfusionMatrix): a dict of Python
    ints na, nb, inter, union, tp, fp, fn.  One device-to-host read."""
    na, nb, inter, union = (int(v) for v in mask_counts_async(a, b).tolist())
    return {"na": na, "nb": nb, "inter": inter, "union": union, "tp": inter, "fp": na - inter, "fn": nb - inter}


def surface_distances(a, b, sampling=(1.0, 1.0, 1.0)):
    """Surface distances between two non-empty masks (utils/surface.Surface): ((sum d, sum d^2, max d, n) of the surface
    voxels of `a` to the surface of `b`, the same of `b` to `a`), d in the units of `sampling` (per axis of the array).
    The distance transforms run over the union bounding box of the two surfaces.  One device-to-host read."""
    a, b = _mask3d(a), _mask3d(b)
    if a.shape != b.shape:
        raise ValueError("shape mismatch: {} and {}".format(tuple(a.shape), tuple(b.shape)))
    sz, sy, sx = (float(v) for v in sampling)
    d, h, w = a.shape
    lib, st, dev = _abi.lib(), stream_ptr(), a.device
    edges = torch.empty((2, d, h, w), dtype=torch.uint8, device=dev)
    box = torch.empty(6, dtype=torch.int32, device=dev)
    check(lib.unetk_surface3d(ptr(a), d, h, w, ptr(edges[0]), ptr(box), 0, st), "surface3d")
    check(lib.unetk_surface3d(ptr(b), d, h, w, ptr(edges[1]), ptr(box), 1, st), "surface3d")
    dist2 = torch.empty((d, h, w), dtype=torch.float64, device=dev)
    n_edt = lib.unetk_edt3d_sq_ws_bytes(d, h, w)
    n_sum = lib.unetk_surface_dist_ws_bytes(d, h, w)
    ws = torch.empty(max(n_edt, n_sum, 16), dtype=torch.uint8, device=dev)
    res = torch.empty((2, 4), dtype=torch.float64, device=dev)
    for k, (src, dst) in enumerate(((0, 1), (1, 0))):     # k = 0: a's surface against b's transform
        check(lib.unetk_edt3d_sq(ptr(edges[dst]), d, h, w, ptr(box), sz, sy, sx, ptr(dist2), ptr(ws), n_edt, st), "edt3d_sq")
        check(lib.unetk_surface_dist(ptr(edges[src]), ptr(dist2), d, h, w, ptr(res[k]), ptr(ws), n_sum, st), "surface_dist")
    host = res.cpu()
    n = host.view(torch.int64)[:, 3].tolist()
    vals = host.tolist()
    return tuple((vals[k][0], vals[k][1], vals[k][2], int(n[k])) for k in range(2))


# ----------------------------------------------------------------------------- offline evaluation I/O (csrc/evalio.hip)
def _device_table(t, dtype, n, device, what):
    """A host array or a device tensor as a dense device tensor of `n` elements of `dtype` (one upload for a host array)."""
    import numpy as np
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype={torch.int32: np.int32, torch.float32: np.float32}[dtype])).to(device)
    _require_cuda(t)
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError("{}: {} dense elements of {} expected, got {} of {}".format(what, n, dtype, tuple(t.shape), t.dtype))
    return t


def eval_slab(vol, zsrc, taps_y, taps_x, lut, out_hw, channels, window=(-200, 250), out=None):
    """One network input slab f32 [N, H, W, C] from a case's resident raw crop (unetk_eval_slab): vol int16 [d, h, w] on the
    device; zsrc int32 [N, C] the source slice of every sample and channel (-1: a plane of 0.0, -2: a plane of HU 0 passed
    through the window); taps_y = (y0, y1, fy) of H entries and taps_x = (x0, x1, fx) of W entries, the bilinear taps of
    data/lits.cv2_linear_taps; lut f32 [hi - lo + 1] the host's normalisation of every HU value of window = (lo, hi).
    Tables may be host arrays (uploaded here) or device tensors (a caller serving many slabs uploads them once).  Bit-equal
    to the host pipeline (window, then cv2_resize_linear).  out: a dense f32 [N, H, W, C] device tensor to write into."""
    _require_cuda(vol)
    if vol.dtype != torch.int16 or vol.dim() != 3 or not vol.is_contiguous():
        raise ValueError("a dense int16 [d, h, w] volume expected, got {} {}".format(vol.dtype, tuple(vol.shape)))
    h, w = int(out_hw[0]), int(out_hw[1])
    c = int(channels)
    lo, hi = int(window[0]), int(window[1])
    dev = vol.device
    n = int(zsrc.shape[0])
    if tuple(zsrc.shape) != (n, c):
        raise ValueError("zsrc must be [N, {}], got {}".format(c, tuple(zsrc.shape)))
    zsrc = _device_table(zsrc, torch.int32, n * c, dev, "zsrc")
    y0, y1 = (_device_table(t, torch.int32, h, dev, "taps_y") for t in taps_y[:2])
    x0, x1 = (_device_table(t, torch.int32, w, dev, "taps_x") for t in taps_x[:2])
    fy = _device_table(taps_y[2], torch.float32, h, dev, "taps_y")
    fx = _device_table(taps_x[2], torch.float32, w, dev, "taps_x")
    lut = _device_table(lut, torch.float32, int(lut.shape[0]) if hasattr(lut, "shape") else len(lut), dev, "lut")
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
    _require_cuda(out)
    if out.dtype != torch.float32 or tuple(out.shape) != (n, h, w, c) or not out.is_contiguous():
        raise ValueError("out must be a dense f32 {} tensor".format((n, h, w, c)))
    d, sh, sw = (int(s) for s in vol.shape)
    with _timed_hbm("eval_slab", out, 1, 2 * 4 * out.numel()):           # the store + four int16 taps per element
        check(_abi.lib().unetk_eval_slab(ptr(vol), d, sh, sw, ptr(zsrc), n, c, ptr(y0), ptr(y1), ptr(fy), h, ptr(x0), ptr(x1),
                                         ptr(fx), w, ptr(lut), lut.numel(), lo, hi, ptr(out), stream_ptr()), "eval_slab")
    return out


_ZOOM_TABLES = {}


def zoom_tables(in_shape, out_shape):
    """Host side of zoom_nearest3d: per axis the int32 source index of every output sample of
    scipy.ndimage.zoom(volume, np.array(out_shape) / np.array(in_shape), order=0), -1 where scipy's sample lands just
    outside the input and becomes cval = 0 (the last sample of an axis for many size pairs: 32 -> 16, 64 -> 93, ...).
    The order-0 zoom is separable, so the tables are asked of the installed scipy itself, axis by axis: the zoom of
    1 .. n_in."""
    import numpy as np
    import scipy.ndimage as ndi
    in_shape, out_shape = tuple(int(s) for s in in_shape), tuple(int(s) for s in out_shape)
    if len(in_shape) != len(out_shape) or min(in_shape + out_shape) <= 0:
        raise ValueError("zoom_tables: positive shapes of one rank expected, got {} and {}".format(in_shape, out_shape))
    key = (in_shape, out_shape)
    if key not in _ZOOM_TABLES:
        scales = np.array(out_shape) / np.array(in_shape)                  # the evaluator's own expression
        tables = []
        for n_in, n_out, s in zip(in_shape, out_shape, scales):
            t = np.rint(ndi.zoom(np.arange(1, n_in + 1, dtype=np.float64), s, order=0)).astype(np.int32) - 1
            assert t.shape == (n_out,), (n_in, n_out, t.shape)
            assert t.min() >= -1 and t.max() < n_in, (n_in, n_out)
            tables.append(t)
        if len(_ZOOM_TABLES) >= 256:
            _ZOOM_TABLES.clear()
        _ZOOM_TABLES[key] = tuple(tables)
    return _ZOOM_TABLES[key]


def zoom_nearest3d(vol_u8, out_shape, tables=None, out=None):
    """scipy.ndimage.zoom(volume, out_shape / volume.shape, order=0) of a uint8 [d, h, w] device volume on the device
    (unetk_zoom_nearest3d), voxel for voxel including scipy's zero samples just outside the input.  tables: the three host
    index tables of zoom_tables (built when None); they are validated here and uploaded in one copy.  out: a dense uint8
    device tensor of out_shape to write into."""
    import numpy as np
    _require_cuda(vol_u8)
    if vol_u8.dtype != torch.uint8 or vol_u8.dim() != 3:
        raise ValueError("a uint8 [d, h, w] volume expected, got {} {}".format(vol_u8.dtype, tuple(vol_u8.shape)))
    vol_u8 = vol_u8.contiguous()
    in_shape = tuple(int(s) for s in vol_u8.shape)
    out_shape = tuple(int(s) for s in out_shape)
    if tables is None:
        tables = zoom_tables(in_shape, out_shape)
    tables = [np.ascontiguousarray(t, dtype=np.int32) for t in tables]
    if len(tables) != 3 or len(out_shape) != 3:
        raise ValueError("three tables and a 3-D output shape expected")
    for t, n_in, n_out in zip(tables, in_shape, out_shape):
        if t.shape != (n_out,) or t.min() < -1 or t.max() >= n_in:
            raise ValueError("zoom table of {} entries in [-1, {}) expected, got {} in [{}, {}]".format(
                n_out, n_in, t.shape, t.min() if t.size else None, t.max() if t.size else None))
    tabs = torch.from_numpy(np.concatenate(tables)).to(vol_u8.device)
    dd, hh, ww = out_shape
    if out is None:
        out = torch.empty(out_shape, dtype=torch.uint8, device=vol_u8.device)
    _require_cuda(out)
    if out.dtype != torch.uint8 or tuple(out.shape) != out_shape or not out.is_contiguous():
        raise ValueError("out must be a dense uint8 {} tensor".format(out_shape))
    with _timed_hbm("zoom_nearest3d", out, 2):                          # one gathered read and one store per output voxel
        check(_abi.lib().unetk_zoom_nearest3d(ptr(vol_u8), in_shape[0], in_shape[1], in_shape[2], ptr(tabs), ptr(tabs[dd:]),
                                              ptr(tabs[dd + hh:]), dd, hh, ww, ptr(out), stream_ptr()), "zoom_nearest3d")
    return out


def nii_compose(liver, tumor, origin, case_shape, trans_bk=(2, 1, 0), flips=(False, False, False), out=None):
    """The saved prediction of one case in NIfTI file order (unetk_nii_compose): liver / tumor are the post-processed uint8
    (or bool) device masks [bd, bh, bw] of the box at origin = (z1, y1, x1) of a case_shape = (d, h, w) volume; either may be
    None.  trans_bk and flips = (flip_x, flip_y, flip_z) are what nii_kits.write_nii applies (nii_kits.file_orientation).
    Returns the flat int16 device tensor of d * h * w elements, file axis 0 fastest: liver + tumor inside the box, 0 outside
    -- np.pad and write_nii's flips, transpose and cast in one pass.  out: a dense int16 tensor of that size to write into."""
    masks = [None if m is None else _mask_bytes(m) for m in (liver, tumor)]
    ref = masks[0] if masks[0] is not None else masks[1]
    if ref is None:
        raise ValueError("nii_compose needs a liver or a tumor mask")
    if masks[1] is not None and masks[1].shape != ref.shape:
        raise ValueError("shape mismatch: {} and {}".format(tuple(ref.shape), tuple(masks[1].shape)))
    bd, bh, bw = (int(s) for s in ref.shape)
    z1, y1, x1 = (int(v) for v in origin)
    d, h, w = (int(v) for v in case_shape)
    tb = tuple(int(v) for v in trans_bk)
    if sorted(tb) != [0, 1, 2]:
        raise ValueError("trans_bk must be a permutation of (0, 1, 2), got {}".format(trans_bk))
    fx, fy, fz = (bool(f) for f in flips)
    if out is None:
        out = torch.empty(d * h * w, dtype=torch.int16, device=ref.device)
    _require_cuda(out)
    if out.dtype != torch.int16 or out.numel() != d * h * w or not out.is_contiguous():
        raise ValueError("out must be a dense int16 tensor of {} elements".format(d * h * w))
    with _timed_hbm("nii_compose", out, 1, sum(m.numel() for m in masks if m is not None)):
        check(_abi.lib().unetk_nii_compose(ptr(masks[0]), ptr(masks[1]), bd, bh, bw, z1, y1, x1, d, h, w, tb[0], tb[1], tb[2],
                                           int(fx) | int(fy) << 1 | int(fz) << 2, ptr(out), stream_ptr()), "nii_compose")
    return out


NII_INGEST_CODES = {"uint8": 2, "int16": 4, "int32": 8, "float32": 16, "float64": 64, "int8": 256, "uint16": 512, "uint32": 768}
STORE_WINDOW = (-250, 300, 64)      # (lo, hi, scale) of the slice store's pixels: DataLoader/Liver/extract.py:32-35


def nii_ingest(block, dtype, file_shape, trans_bk=(2, 1, 0), flips=(False, False, False), slope=0.0, inter=0.0, out=None,
               window=STORE_WINDOW):
    """A NIfTI file's voxel block as store slices (unetk_nii_ingest): block = the file's bytes behind
    vox_offset on the device (a dense uint8 tensor of at least prod(file_shape) * itemsize bytes, little-endian), dtype its
    numpy datatype name, file_shape = (n0, n1, n2) with axis 0 fastest; trans_bk and flips = (flip_x, flip_y, flip_z) are
    nii_kits.file_orientation's.  slope / inter: the header's scl_slope / scl_inter (applied when the slope is neither 0 nor
    NaN).  Returns the int16-typed storage [d, h, w] of the uint16 pixels (clip(int16(v), lo, hi) - lo) * scale, bit for bit
    what nii_kits.read_nii and the store's encoding give.  out: a dense int16 [d, h, w] tensor to write into."""
    _require_cuda(block)
    name = str(getattr(dtype, "name", dtype))
    if name not in NII_INGEST_CODES:
        raise ValueError("unsupported NIfTI datatype {}".format(dtype))
    item = {2: 1, 256: 1, 4: 2, 512: 2, 8: 4, 16: 4, 768: 4, 64: 8}[NII_INGEST_CODES[name]]
    n0, n1, n2 = (int(v) for v in file_shape)
    if block.dtype != torch.uint8 or block.dim() != 1 or not block.is_contiguous() or block.numel() < n0 * n1 * n2 * item:
        raise ValueError("a dense 1-D uint8 tensor of at least {} bytes expected".format(n0 * n1 * n2 * item))
    tb = tuple(int(v) for v in trans_bk)
    if sorted(tb) != [0, 1, 2]:
        raise ValueError("trans_bk must be a permutation of (0, 1, 2), got {}".format(trans_bk))
    zyx = [0, 0, 0]
    for k, axis in enumerate(tb):
        zyx[axis] = (n0, n1, n2)[k]
    fx, fy, fz = (bool(f) for f in flips)
    lo, hi, scale = (int(v) for v in window)
    if out is None:
        out = torch.empty(tuple(zyx), dtype=torch.int16, device=block.device)
    _require_cuda(out)
    if out.dtype != torch.int16 or tuple(out.shape) != tuple(zyx) or not out.is_contiguous():
        raise ValueError("out must be a dense int16 {} tensor".format(tuple(zyx)))
    with _timed_hbm("nii_ingest", out, 1, n0 * n1 * n2 * item):        # the block read once, the slices written once
        check(_abi.lib().unetk_nii_ingest(ptr(block), NII_INGEST_CODES[name], n0, n1, n2, float(slope), float(inter), tb[0], tb[1],
                                          tb[2], int(fx) | int(fy) << 1 | int(fz) << 2, lo, hi, scale, ptr(out), stream_ptr()),
              "nii_ingest")
    return out


def _mask_bytes(t):
    """A [D, H, W] device mask as dense bytes, values kept (bool -> 0 / 1)."""
    _require_cuda(t)
    if t.dim() != 3:
        raise ValueError("a 3-D [D, H, W] mask expected, got shape {}".format(tuple(t.shape)))
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        raise ValueError("a uint8 or bool mask expected, got {}".format(t.dtype))
    return t.contiguous()


GUIDE_ROW = 12            # int32 words per component row of unetk_guide_components


def guide_components_ws(h, w, cap, device):
    """A workspace for guide_components at [h, w] with table capacity cap (one per loop: it is reused every slice)."""
    nbytes = _abi.lib().unetk_guide_components_ws_bytes(int(h), int(w), int(cap))
    if nbytes == 0:
        raise ValueError("unsupported guide_components shape {}x{} / capacity {}".format(h, w, cap))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def guide_components(acc, guide, cap=1024, table=None, ws=None):
    """The tumour components of one slice of the guide propagation (unetk_guide_components): acc f32 [H, W, 3] the
    mirror-averaged probabilities, guide f32 [H, W] the guide the slice was given.  Returns the int32 device table
    [4 + cap * GUIDE_ROW]: head {count, overflow, 0, 0}, then per component in root order {root, area, y0, x0, y1, x1, peak
    index, peak value, cy, cx, sy, sx} (the last five are float32 bits).  No host read; runs on the current stream."""
    _require_cuda(acc, guide)
    h, w = int(acc.shape[0]), int(acc.shape[1])
    assert acc.dtype == torch.float32 and tuple(acc.shape) == (h, w, 3) and acc.is_contiguous()
    assert guide.dtype == torch.float32 and guide.numel() == h * w and guide.is_contiguous()
    if table is None:
        table = torch.empty(4 + cap * GUIDE_ROW, dtype=torch.int32, device=acc.device)
    assert table.dtype == torch.int32 and table.numel() >= 4 + cap * GUIDE_ROW and table.is_contiguous()
    nbytes = _abi.lib().unetk_guide_components_ws_bytes(h, w, int(cap))
    if ws is None:
        ws = guide_components_ws(h, w, cap, acc.device)
    assert ws.numel() >= nbytes
    check(_abi.lib().unetk_guide_components(ptr(acc), ptr(guide), h, w, int(cap), ptr(table), ptr(ws), nbytes, stream_ptr()),
          "guide_components")
    return table


def guide_render(obj, out_hw, discount, out=None):
    """The guide f32 [H, W] of one propagation slice (unetk_guide_render): obj f32 [n, 4] = (cy, cx, sy, sx) on the device
    (16-byte aligned rows), max of the Gaussians x discount / 2 + 0.5; exactly 0.5 without objects."""
    h, w = int(out_hw[0]), int(out_hw[1])
    n = 0 if obj is None else int(obj.shape[0])
    if n:
        _require_cuda(obj)
        assert obj.dtype == torch.float32 and obj.dim() == 2 and obj.shape[1] == 4 and obj.is_contiguous()
    if out is None:
        out = torch.empty((h, w), dtype=torch.float32, device=obj.device if n else torch.device("cuda", torch.cuda.current_device()))
    assert out.dtype == torch.float32 and out.numel() == h * w and out.is_contiguous()
    check(_abi.lib().unetk_guide_render(ptr(obj) if n else None, n, h, w, float(discount), ptr(out), stream_ptr()),
          "guide_render")
    return out


def lits_batch(slices, seg_slices, sample_tab, clip, out_hw, channels, lab_scale=64, noise_scale=0.0, seed=0):
    """One training batch from device-resident decoded slices (input_pipeline.py:243-284): slices uint16 / seg_slices
    uint8 [n, src_h, src_w] (stored as int16 / uint8 tensors), sample_tab int32 [N, C+7], clip f32 [N, 2]."""
    _require_cuda(slices, seg_slices, sample_tab, clip)
    n = sample_tab.shape[0]
    h, w = out_hw
    assert slices.dtype in (torch.int16, torch.uint16) and seg_slices.dtype == torch.uint8
    assert sample_tab.dtype == torch.int32 and sample_tab.shape[1] == channels + 7 and sample_tab.is_contiguous()
    assert clip.dtype == torch.float32 and tuple(clip.shape) == (n, 2) and clip.is_contiguous()
    assert slices.is_contiguous() and seg_slices.is_contiguous() and slices.shape == seg_slices.shape
    d = _abi.LitsDesc(n, h, w, channels, slices.shape[0], slices.shape[1], slices.shape[2], int(lab_scale),
                      int(seed) & 0xffffffff, float(noise_scale))
    images = torch.empty((n, h, w, channels), dtype=torch.float32, device=slices.device)
    labels = torch.empty((n, h, w), dtype=torch.int32, device=slices.device)
    check(_abi.lib().unetk_lits_batch(ctypes.byref(d), ptr(slices), ptr(seg_slices), ptr(sample_tab), ptr(clip), ptr(images),
                                      ptr(labels), stream_ptr()), "lits_batch")
    return images, labels


def lits_spatial_guide(tab, obj_ptr, obj, out_hw, channels, src_hw, min_std=1.0):
    """The spatial guide f32 [N, H, W, 1] of a batch (input_pipeline_g.py:382-412, unetk_lits_spatial_guide): tab = the
    batch's int32 [N, C+7] table of lits_batch (crop boxes and flips), obj_ptr int32 [N + 1] CSR into obj f32 [M, 4] =
    (cy, cx, sy, sx), centres relative to the crop; stddevs floored at min_std.  Runs on the current stream."""
    _require_cuda(tab, obj_ptr)
    n = tab.shape[0]
    h, w = out_hw
    assert tab.dtype == torch.int32 and tab.dim() == 2 and tab.shape[1] == channels + 7 and tab.is_contiguous()
    assert obj_ptr.dtype == torch.int32 and tuple(obj_ptr.shape) == (n + 1,) and obj_ptr.is_contiguous()
    assert obj.dtype == torch.float32 and obj.dim() == 2 and obj.shape[1] == 4 and obj.is_contiguous()
    m = obj.shape[0]
    if m:
        _require_cuda(obj)
    d = _abi.LitsGuideDesc(n, h, w, channels, int(src_hw[0]), int(src_hw[1]), m, float(min_std))
    guide = torch.empty((n, h, w, 1), dtype=torch.float32, device=tab.device)
    check(_abi.lib().unetk_lits_spatial_guide(ctypes.byref(d), ptr(tab), ptr(obj_ptr), ptr(obj) if m else None, ptr(guide),
                                              stream_ptr()), "lits_spatial_guide")
    return guide


def lits_context(table, tab, channels, take, noise=None):
    """The context rows f32 [N, F] of a batch (unetk_lits_context): row s = table[tab[s, channels]] where take[s] != 0 and
    the index is a row of `table`, else zeros.  noise f64 [N, F]: the table rows are first updated in place,
    row = f32(f64(row) + noise[s]), samples in order.  All on the device; runs on the current stream."""
    _require_cuda(table, tab, take)
    n = tab.shape[0]
    assert table.dtype == torch.float32 and table.dim() == 2 and table.is_contiguous()
    assert tab.dtype == torch.int32 and tab.dim() == 2 and tab.shape[1] == channels + 7 and tab.is_contiguous()
    assert take.dtype == torch.int32 and tuple(take.shape) == (n,) and take.is_contiguous()
    f = table.shape[1]
    if noise is not None:
        _require_cuda(noise)
        assert noise.dtype == torch.float64 and tuple(noise.shape) == (n, f) and noise.is_contiguous()
    out = torch.empty((n, f), dtype=torch.float32, device=tab.device)
    check(_abi.lib().unetk_lits_context(ptr(table), table.shape[0], f, ptr(tab), n, channels, ptr(take),
                                        ptr(noise) if noise is not None else None, ptr(out), stream_ptr()), "lits_context")
    return out


def lits_pick_voxels(seg_slices, sample_tab, fg_label, status, lab_scale=64):
    """The forced-class centres of a 3-D batch (unetk_lits_pick_voxel): every row of sample_tab int32 [N, 16] with
    forced != 0 gets (cy, cx) = np.argwhere(seg_slices[base + cz] / lab_scale >= fg_label)[k], written IN PLACE on the
    device; status int32 [1] (zeroed by the caller) gets bit 0 for a k beyond the slice's count.  Current stream."""
    _require_cuda(seg_slices, sample_tab, status)
    assert seg_slices.dtype == torch.uint8 and seg_slices.dim() == 3 and seg_slices.is_contiguous()
    assert sample_tab.dtype == torch.int32 and sample_tab.dim() == 2 and sample_tab.shape[1] == _abi.LITS3D_TAB_COLS
    assert sample_tab.is_contiguous() and status.dtype == torch.int32 and status.numel() >= 1
    with _timed_hbm("lits_pick_voxels", seg_slices[0], sample_tab.shape[0]):          # at most one label slice per sample
        check(_abi.lib().unetk_lits_pick_voxel(ptr(seg_slices), seg_slices.shape[0], seg_slices.shape[1], seg_slices.shape[2],
                                               int(lab_scale), int(fg_label), ptr(sample_tab), sample_tab.shape[0], ptr(status),
                                               stream_ptr()), "lits_pick_voxels")
    return sample_tab


def lits_pick_voxel_rows(plane, sample_tab, forced_value, status, fg_label=1, lab_scale=64):
    """`lits_pick_voxels` for the rows whose column 11 equals forced_value only (unetk_lits_pick_voxel_rows): one table serves
    rows centred on the label plane (value 1) and rows centred on the `neg` plane (value 2, label 1), one call per plane.  A
    rank beyond the slice's count sets status bit 0, and bit 1 too when forced_value > 1.  Current stream."""
    _require_cuda(plane, sample_tab, status)
    assert plane.dtype == torch.uint8 and plane.dim() == 3 and plane.is_contiguous()
    assert sample_tab.dtype == torch.int32 and sample_tab.dim() == 2 and sample_tab.shape[1] == _abi.LITS3D_TAB_COLS
    assert sample_tab.is_contiguous() and status.dtype == torch.int32 and status.numel() >= 1
    with _timed_hbm("lits_pick_voxel_rows", plane[0], sample_tab.shape[0]):
        check(_abi.lib().unetk_lits_pick_voxel_rows(ptr(plane), plane.shape[0], plane.shape[1], plane.shape[2], int(lab_scale),
                                                    int(fg_label), ptr(sample_tab), sample_tab.shape[0], ptr(status),
                                                    int(forced_value), stream_ptr()), "lits_pick_voxel_rows")
    return sample_tab


def lits3d_desc(slices, n, shape, training, lab_max=2, im_scale=64, lab_scale=64):
    d, h, w = (int(v) for v in shape)
    return _abi.Lits3dDesc(int(n), d, h, w, slices.shape[0], slices.shape[1], slices.shape[2], int(im_scale), int(lab_scale),
                           int(lab_max), 1 if training else 0)


def _warp_lattice(warp, grid, n, device):
    """The checks of a `warp=` argument: f32 [n, 2, G + 3, G + 3] on the table's device, 1 <= G <= 16 -> G."""
    g = int(grid)
    if not 1 <= g <= 16:
        raise ValueError("grid must satisfy 1 <= G <= 16, got {}".format(grid))
    _require_cuda(warp)
    assert warp.dtype == torch.float32 and tuple(warp.shape) == (n, 2, g + 3, g + 3) and warp.is_contiguous(), \
        (warp.dtype, tuple(warp.shape), (n, 2, g + 3, g + 3))
    assert warp.device == device
    return g


def _zcrop_args(name, zcrop, zcrop_max, n, device, slices):
    """The checks of a `zcrop=` argument: int32 [n] on the table's device and zcrop_max, the largest crop
    depth the host put there -> int(zcrop_max); zcrop_max * src_h * src_w must index in 31 bits."""
    _require_cuda(zcrop)
    assert zcrop.dtype == torch.int32 and tuple(zcrop.shape) == (n,) and zcrop.is_contiguous() and zcrop.device == device
    zmax = int(zcrop_max)
    if zmax < 1:
        raise ValueError("{}: zcrop_max must be >= 1, got {}".format(name, zcrop_max))
    if zmax * int(slices.shape[1]) * int(slices.shape[2]) >= 1 << 31 or zmax >= 1 << 24:
        raise _abi.UnetkError("{}: a crop of {} slices of {} x {} is beyond 31-bit indexing".format(name, zmax, slices.shape[1],
                                                                                                 slices.shape[2]))
    return zmax


def lits_patch3d(slices, seg_slices, sample_tab, shape, training, lab_max=2, im_scale=64, lab_scale=64, rotate=False, warp=None,
                 grid=0, zcrop=None, zcrop_max=0):
    """One UNet3D batch from the device-resident slice store (unetk_lits_patch3d; include/unetk.h has the table layout):
    slices uint16 / seg_slices uint8 [n, src_h, src_w] (stored as int16 / uint8 tensors), sample_tab int32 [N, 16],
    shape = (D, H, W).  Returns images f32 [N, D, H, W, 1], labels int32 [N, D, H, W].  training: gamma augmentation with
    the table's per-sample gamma.  rotate: unetk_lits_patch3d_rot, which turns the rows whose columns 13 / 14 hold (sin, cos)
    in the plane; without it the columns are ignored.  warp f32 [N, 2, grid + 3, grid + 3]:
    unetk_lits_patch3d_warp, which also deforms the rows whose column 15 is not zero by their B-spline lattice of `grid` cells
    per axis and reads the rotation columns whatever `rotate` says.  zcrop int32 [N] with zcrop_max, its
    largest entry: unetk_lits_patch3d_z, which resizes min(max(zcrop[n], 1), zcrop_max) crop slices of row n to the D output
    slices (not together with rotate / warp).  Current stream; no host synchronisation."""
    if zcrop is not None and (rotate or warp is not None):
        raise ValueError("lits_patch3d: zcrop is not served together with rotate or warp (DESIGN.md 7.3.17)")
    _require_cuda(slices, seg_slices, sample_tab)
    assert slices.dtype in (torch.int16, torch.uint16) and seg_slices.dtype == torch.uint8
    assert slices.is_contiguous() and seg_slices.is_contiguous() and slices.shape == seg_slices.shape and slices.dim() == 3
    assert sample_tab.dtype == torch.int32 and sample_tab.dim() == 2 and sample_tab.shape[1] == _abi.LITS3D_TAB_COLS
    assert sample_tab.is_contiguous()
    n = sample_tab.shape[0]
    desc = lits3d_desc(slices, n, shape, training, lab_max, im_scale, lab_scale)
    nbytes = int(_abi.lib().unetk_lits_patch3d_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("lits_patch3d: unsupported shape {} from {} x {} slices".format(tuple(shape), slices.shape[1],
                                                                                              slices.shape[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=slices.device)
    images = torch.empty((n, desc.D, desc.H, desc.W, 1), dtype=torch.float32, device=slices.device)
    labels = torch.empty((n, desc.D, desc.H, desc.W), dtype=torch.int32, device=slices.device)
    # algorithmic bytes: the image written once (training: + the two gamma passes' read and write) and the labels; the crop
    # reads depend on the table's zoom and are left out
    name = "lits_patch3d_warp" if warp is not None else "lits_patch3d_rot" if rotate else "lits_patch3d"
    lattice = () if warp is None else (ptr(warp), _warp_lattice(warp, grid, n, sample_tab.device))
    if zcrop is not None:
        name, lattice = "lits_patch3d_z", (ptr(zcrop), _zcrop_args("lits_patch3d", zcrop, zcrop_max, n, sample_tab.device, slices))
    with _timed_hbm(name, images, 5 if training else 1, labels.numel() * 4):
        check(getattr(_abi.lib(), "unetk_" + name)(ctypes.byref(desc), ptr(slices), ptr(seg_slices), ptr(sample_tab), *lattice,
                                                   ptr(images), ptr(labels), ptr(ws), nbytes, stream_ptr()), name)
    return images, labels


def _eval3d_accumulate_args(name, probs, sample_tab, shape, case_base, case_depth, box, acc, weight, weight_dtype, slices,
                            host_tab):
    """The checks the two accumulate wrappers share -> (desc, c, cbox, voxels of the box)."""
    _require_cuda(probs, sample_tab, acc, weight, slices)
    d, h, w = (int(v) for v in shape)
    assert sample_tab.dtype == torch.int32 and sample_tab.dim() == 2 and sample_tab.shape[1] == _abi.LITS3D_TAB_COLS
    assert sample_tab.is_contiguous()
    n = sample_tab.shape[0]
    assert probs.dtype == torch.float32 and probs.dim() == 5 and tuple(probs.shape[:4]) == (n, d, h, w) and probs.is_contiguous()
    c = int(probs.shape[4])
    assert slices.dim() == 3
    vol = (int(case_depth), int(slices.shape[1]), int(slices.shape[2]))
    assert acc.dtype == torch.float32 and tuple(acc.shape) == vol + (c,) and acc.is_contiguous()
    assert weight.dtype == weight_dtype and tuple(weight.shape) == vol and weight.is_contiguous()
    if host_tab is not None:
        rows = torch.as_tensor(host_tab)
        if tuple(rows.shape) != (n, _abi.LITS3D_TAB_COLS) or bool((rows[:, 0] != int(case_base)).any()) or \
                bool((rows[:, 1] != int(case_depth)).any()):
            raise _abi.UnetkError("{}: every row must carry the case's (base, depth) = ({}, {})".format(
                name, int(case_base), int(case_depth)))
        if bool((rows[:, 13:15] != 0).any()):
            raise ValueError("{}: a row carries a rotation (columns 13 / 14 of the table): a rotated window cannot be "
                             "accumulated back into its case".format(name))
        if bool((rows[:, 15] != 0).any()):
            raise ValueError("{}: a row is deformed (column 15 of the table): a deformed window cannot be accumulated back "
                             "into its case".format(name))
    desc = lits3d_desc(slices, n, shape, False)
    cbox = (ctypes.c_int32 * 6)(*(int(v) for v in box))
    return desc, c, cbox, (cbox[1] - cbox[0]) * (cbox[3] - cbox[2]) * (cbox[5] - cbox[4])


def eval3d_accumulate(probs, sample_tab, shape, case_base, case_depth, box, acc, cnt, slices, host_tab=None, zcrop=None,
                      zcrop_max=0):
    """Window probabilities back into ONE case at source resolution (unetk_eval3d_accumulate): probs f32
    [N, D, H, W, C] of the windows `lits_patch3d(..., training=False)` cut for sample_tab int32 [N, 16]; acc f32
    [depth, src_h, src_w, C] and cnt int32 [depth, src_h, src_w] are updated IN PLACE (the caller zeroes them before the
    case's first batch); box = (z0, z1, y0, y1, x0, x1), the union of the rows' crop boxes; slices: the resident store the
    windows were cut from (its extent enters the crop box).  host_tab: the table's host copy, when the caller has it -- the
    rows' (base, depth) are then checked against the case here (a device table is not read back), and a row with a rotation
    in columns 13 / 14 raises ValueError (the kernels ignore those columns).  zcrop int32 [N] with zcrop_max: the windows
    `lits_patch3d(..., zcrop=zcrop, zcrop_max=zcrop_max)` cut (unetk_eval3d_accumulate_z), box the union of
    their cd-deep crop boxes.  Current stream; no host synchronisation."""
    desc, c, cbox, nvox = _eval3d_accumulate_args("eval3d_accumulate", probs, sample_tab, shape, case_base, case_depth, box, acc,
                                                  cnt, torch.int32, slices, host_tab)
    if zcrop is not None:
        zmax = _zcrop_args("eval3d_accumulate", zcrop, zcrop_max, sample_tab.shape[0], sample_tab.device, slices)
        with _timed_hbm("eval3d_accumulate_z", probs, 1, nvox * 8 * (c + 1)):
            check(_abi.lib().unetk_eval3d_accumulate_z(ctypes.byref(desc), ptr(sample_tab), ptr(zcrop), zmax, ptr(probs), c,
                                                       int(case_base), int(case_depth), cbox, ptr(acc), ptr(cnt), stream_ptr()),
                  "eval3d_accumulate_z")
        return acc, cnt
    # algorithmic bytes: the windows read once, the box of acc read and written, the box of cnt read and written
    with _timed_hbm("eval3d_accumulate", probs, 1, nvox * 8 * (c + 1)):
        check(_abi.lib().unetk_eval3d_accumulate(ctypes.byref(desc), ptr(sample_tab), ptr(probs), c, int(case_base),
                                                 int(case_depth), cbox, ptr(acc), ptr(cnt), stream_ptr()), "eval3d_accumulate")
    return acc, cnt


def eval3d_accumulate_w(probs, sample_tab, shape, case_base, case_depth, box, tables, acc, wsum, slices, host_tab=None, zcrop=None,
                        zcrop_max=0):
    """eval3d_accumulate with centre-weighted windows (unetk_eval3d_accumulate_w; --eval_window_weight gaussian): tables =
    (gz f32 [D], gy f32 [H], gx f32 [W]) device vectors (data/lits3d.window_weights); wsum f32 [depth, src_h, src_w] takes
    the place of cnt and collects the weights.  Everything else as eval3d_accumulate (zcrop: unetk_eval3d_accumulate_wz)."""
    desc, c, cbox, nvox = _eval3d_accumulate_args("eval3d_accumulate_w", probs, sample_tab, shape, case_base, case_depth, box, acc,
                                                  wsum, torch.float32, slices, host_tab)
    gz, gy, gx = tables
    _require_cuda(gz, gy, gx)
    for g, n in zip((gz, gy, gx), shape):
        assert g.dtype == torch.float32 and tuple(g.shape) == (int(n),) and g.is_contiguous()
    if zcrop is not None:
        zmax = _zcrop_args("eval3d_accumulate_w", zcrop, zcrop_max, sample_tab.shape[0], sample_tab.device, slices)
        with _timed_hbm("eval3d_accumulate_wz", probs, 1, nvox * 8 * (c + 1) + 4 * (gz.numel() + gy.numel() + gx.numel())):
            check(_abi.lib().unetk_eval3d_accumulate_wz(ctypes.byref(desc), ptr(sample_tab), ptr(zcrop), zmax, ptr(probs), c,
                                                        int(case_base), int(case_depth), cbox, ptr(gz), ptr(gy), ptr(gx), ptr(acc),
                                                        ptr(wsum), stream_ptr()), "eval3d_accumulate_wz")
        return acc, wsum
    # algorithmic bytes: as eval3d_accumulate with wsum for cnt, and the three tables once
    with _timed_hbm("eval3d_accumulate_w", probs, 1, nvox * 8 * (c + 1) + 4 * (gz.numel() + gy.numel() + gx.numel())):
        check(_abi.lib().unetk_eval3d_accumulate_w(ctypes.byref(desc), ptr(sample_tab), ptr(probs), c, int(case_base),
                                                   int(case_depth), cbox, ptr(gz), ptr(gy), ptr(gx), ptr(acc), ptr(wsum),
                                                   stream_ptr()), "eval3d_accumulate_w")
    return acc, wsum


def eval3d_finish(acc, weight, box, uncovered):
    """The end of a sliding-window case (unetk_eval3d_finish): acc f32 [depth, src_h, src_w, C]; weight: wsum f32 or cnt
    int32 [depth, src_h, src_w]; box = (z0, z1, y0, y1, x0, x1), the part of the case the windows tiled.  Returns pred uint8
    [depth, src_h, src_w]: the argmax over the C sums (lowest index on ties, as head_predict) where the weight is positive
    inside the box, else 0.  uncovered int32 [1] (zeroed by the caller) is raised by the number of voxels of the box
    without cover; it is NOT read here.  Current stream."""
    _require_cuda(acc, weight, uncovered)
    assert acc.dtype == torch.float32 and acc.dim() == 4 and acc.is_contiguous()
    assert weight.dtype in (torch.float32, torch.int32) and tuple(weight.shape) == tuple(acc.shape[:3]) and weight.is_contiguous()
    assert uncovered.dtype == torch.int32 and uncovered.numel() >= 1
    depth, src_h, src_w, c = (int(v) for v in acc.shape)
    pred = torch.empty((depth, src_h, src_w), dtype=torch.uint8, device=acc.device)
    cbox = (ctypes.c_int32 * 6)(*(int(v) for v in box))
    is_w = weight.dtype == torch.float32
    # algorithmic bytes: acc and the weight read once, pred written
    with _timed_hbm("eval3d_finish", acc, 1, weight.numel() * 5):
        check(_abi.lib().unetk_eval3d_finish(ptr(acc), c, depth, src_h, src_w, ptr(weight) if is_w else None,
                                             None if is_w else ptr(weight), cbox, ptr(pred), ptr(uncovered), stream_ptr()),
              "eval3d_finish")
    return pred


def eval3d_prob(acc, weight, cls, box=None, trans_bk=(2, 1, 0), flips=(False, False, False), out=None):
    """The probability of class `cls` of a sliding-window case as a saved volume (unetk_eval3d_prob): acc, weight and box as
    eval3d_finish takes them (box None: the whole case).  Returns the flat uint8 device tensor of depth * src_h * src_w
    elements in NIfTI file order (trans_bk, flips = (flip_x, flip_y, flip_z): nii_kits.file_orientation), q = rint(255 * acc /
    weight) clamped to 0..255, and 0 where the weight is not positive or outside the box.  Current stream."""
    _require_cuda(acc, weight)
    assert acc.dtype == torch.float32 and acc.dim() == 4 and acc.is_contiguous()
    assert weight.dtype in (torch.float32, torch.int32) and tuple(weight.shape) == tuple(acc.shape[:3]) and weight.is_contiguous()
    depth, src_h, src_w, c = (int(v) for v in acc.shape)
    tb = tuple(int(v) for v in trans_bk)
    if sorted(tb) != [0, 1, 2]:
        raise ValueError("trans_bk must be a permutation of (0, 1, 2), got {}".format(trans_bk))
    fx, fy, fz = (bool(f) for f in flips)
    if out is None:
        out = torch.empty(depth * src_h * src_w, dtype=torch.uint8, device=acc.device)
    _require_cuda(out)
    if out.dtype != torch.uint8 or out.numel() != depth * src_h * src_w or not out.is_contiguous():
        raise ValueError("out must be a dense uint8 tensor of {} elements".format(depth * src_h * src_w))
    cbox = (ctypes.c_int32 * 6)(*(int(v) for v in (box if box is not None else (0, depth, 0, src_h, 0, src_w))))
    is_w = weight.dtype == torch.float32
    # algorithmic bytes: one class of acc and the weight read once, the volume written
    with _timed_hbm("eval3d_prob", weight, 2, out.numel()):
        check(_abi.lib().unetk_eval3d_prob(ptr(acc), c, int(cls), depth, src_h, src_w, ptr(weight) if is_w else None,
                                           None if is_w else ptr(weight), cbox, tb[0], tb[1], tb[2],
                                           int(fx) | int(fy) << 1 | int(fz) << 2, ptr(out), stream_ptr()), "eval3d_prob")
    return out


def lits_inter_desc(slices, n, shape, training=False, obj_label=1, im_scale=64, lab_scale=64, noise_scale=0.0, seed=0,
                    clicks=(3, 10, 40, 5)):
    """The descriptor of unetk_lits_inter_batch and unetk_lits_clicks (include/unetk.h): shape = (C, H, W), clicks = (margin,
    step, band, max_clicks) -- the reference's 3, 10, 40, 5 (input_pipeline_g_simply.py:548-560)."""
    c, h, w = (int(v) for v in shape)
    margin, step, band, max_clicks = (int(v) for v in clicks)
    return _abi.LitsInterDesc(N=int(n), H=h, W=w, C=c, n_slices=slices.shape[0], src_h=slices.shape[1], src_w=slices.shape[2],
                              im_scale=int(im_scale), lab_scale=int(lab_scale), obj_label=int(obj_label),
                              training=1 if training else 0, seed=int(seed) & 0xffffffff, noise_scale=float(noise_scale),
                              margin=margin, step=step, band=band, max_clicks=max_clicks, G=2, gaussian=0, stddev=1.0)


def _inter_tab(sample_tab):
    assert sample_tab.dtype == torch.int32 and sample_tab.dim() == 2 and sample_tab.shape[1] == _abi.LITS3D_TAB_COLS
    assert sample_tab.is_contiguous()
    return sample_tab.shape[0]


def lits_inter_batch(slices, seg_slices, sample_tab, shape, training, status, obj_label=1, noise_scale=0.0, seed=0,
                     im_scale=64, lab_scale=64):
    """One click-guided 2-D batch without its guide (unetk_lits_inter_batch): sample_tab int32 [N, 16] (the LiTS 3-D table),
    shape = (C, H, W).  Returns images f32 [N, H, W, C], labels int32 [N, H, W] in {0, 1} (1 = stored label >= obj_label).
    training: gamma with the table's per-sample gamma, then -- noise_scale > 0 -- uniform noise keyed by `seed` and the
    channel mask.  status int32 [1] (zeroed by the caller) collects bit 1; it is NOT read here.  Current stream."""
    _require_cuda(slices, seg_slices, sample_tab, status)
    assert slices.dtype in (torch.int16, torch.uint16) and seg_slices.dtype == torch.uint8
    assert slices.is_contiguous() and seg_slices.is_contiguous() and slices.shape == seg_slices.shape and slices.dim() == 3
    assert status.dtype == torch.int32 and status.numel() >= 1
    n = _inter_tab(sample_tab)
    desc = lits_inter_desc(slices, n, shape, training, obj_label, im_scale, lab_scale, noise_scale, seed)
    nbytes = int(_abi.lib().unetk_lits_inter_batch_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("lits_inter_batch: unsupported shape {} (C odd, <= 7) from {} x {} slices".format(
            tuple(shape), slices.shape[1], slices.shape[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=slices.device)
    images = torch.empty((n, desc.H, desc.W, desc.C), dtype=torch.float32, device=slices.device)
    labels = torch.empty((n, desc.H, desc.W), dtype=torch.int32, device=slices.device)
    with _timed_hbm("lits_inter_batch", images, 7 if training else 1, labels.numel() * 4):
        check(_abi.lib().unetk_lits_inter_batch(ctypes.byref(desc), ptr(slices), ptr(seg_slices), ptr(sample_tab), ptr(images),
                                                ptr(labels), ptr(status), ptr(ws), nbytes, stream_ptr()), "lits_inter_batch")
    return images, labels


def lits_clicks(seg_slices, sample_tab, click_tab, status, obj_label=1, clicks=(3, 10, 40, 5), lab_scale=64):
    """The simulated clicks of a batch (unetk_lits_clicks; include/unetk.h has the semantics): click_tab uint32-valued int32
    [N, 12] = the sample's draws.  Returns pts int32 [N, 2, 4, 2] = (kind fg / bg, click, (y, x) in the crop; -1 padding)
    and cnt int32 [N, 2].  status collects bits 1 and 2; it is NOT read here.  Current stream."""
    _require_cuda(seg_slices, sample_tab, click_tab, status)
    assert seg_slices.dtype == torch.uint8 and seg_slices.dim() == 3 and seg_slices.is_contiguous()
    n = _inter_tab(sample_tab)
    assert click_tab.dtype == torch.int32 and tuple(click_tab.shape) == (n, _abi.LITS_CLICK_TAB_COLS) and click_tab.is_contiguous()
    assert status.dtype == torch.int32 and status.numel() >= 1
    desc = lits_inter_desc(seg_slices, n, (1, 1, 1), obj_label=obj_label, lab_scale=lab_scale, clicks=clicks)
    nbytes = int(_abi.lib().unetk_lits_clicks_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("lits_clicks: unsupported parameters {} on {} x {} slices".format(
            tuple(clicks), seg_slices.shape[1], seg_slices.shape[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=seg_slices.device)
    pts = torch.empty((n, 2, _abi.LITS_MAX_CLICKS, 2), dtype=torch.int32, device=seg_slices.device)
    cnt = torch.empty((n, 2), dtype=torch.int32, device=seg_slices.device)
    with _timed_hbm("lits_clicks", ws, 3):
        check(_abi.lib().unetk_lits_clicks(ctypes.byref(desc), ptr(seg_slices), ptr(sample_tab), ptr(click_tab), ptr(pts),
                                           ptr(cnt), ptr(status), ptr(ws), nbytes, stream_ptr()), "lits_clicks")
    return pts, cnt


def click_guide(sample_tab, pts, cnt, out_hw, src_hw, guide_channel=2, stddev=None):
    """sp_guide f32 [N, H, W, guide_channel] from clicks (unetk_click_guide): pts int32 [N, 2, 4, 2], cnt int32 [N, 2], in the
    crop boxes and under the flips of sample_tab.  stddev None: Euclidean distance to the nearest click; a float: the
    Gaussian of --local_enhance.  guide_channel 2: (fg, bg); 1: fg - bg.  Current stream."""
    _require_cuda(sample_tab, pts, cnt)
    n = _inter_tab(sample_tab)
    assert pts.dtype == torch.int32 and tuple(pts.shape) == (n, 2, _abi.LITS_MAX_CLICKS, 2) and pts.is_contiguous()
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (n, 2) and cnt.is_contiguous()
    h, w = int(out_hw[0]), int(out_hw[1])
    # the guide reads the geometry and its own three fields; the store's and the simulator's only have to be valid
    desc = _abi.LitsInterDesc(N=n, H=h, W=w, C=1, n_slices=1, src_h=int(src_hw[0]), src_w=int(src_hw[1]), im_scale=1, lab_scale=1,
                              obj_label=1, training=0, seed=0, noise_scale=0.0, margin=1, step=0, band=1, max_clicks=2,
                              G=int(guide_channel), gaussian=0 if stddev is None else 1,
                              stddev=0.0 if stddev is None else float(stddev))
    guide = torch.empty((n, h, w, int(guide_channel)), dtype=torch.float32, device=sample_tab.device)
    with _timed_hbm("click_guide", guide, 1):
        check(_abi.lib().unetk_click_guide(ctypes.byref(desc), ptr(sample_tab), ptr(pts), ptr(cnt), ptr(guide), stream_ptr()),
              "click_guide")
    return guide


def click_guide_list(sample_tab, pts, cnt, out_hw, src_hw, guide_channel=2, stddev=None):
    """click_guide from lists of K clicks per kind (unetk_click_guide_list): pts int32 [N, 2, K, 2] with K <= 64, cnt int32
    [N, 2].  The same kernel: bit-equal to click_guide where every count is <= 4.  Current stream."""
    _require_cuda(sample_tab, pts, cnt)
    n = _inter_tab(sample_tab)
    assert pts.dtype == torch.int32 and pts.dim() == 4 and pts.shape[0] == n and pts.shape[1] == 2 and pts.shape[3] == 2
    assert pts.is_contiguous() and cnt.dtype == torch.int32 and tuple(cnt.shape) == (n, 2) and cnt.is_contiguous()
    k = int(pts.shape[2])
    h, w = int(out_hw[0]), int(out_hw[1])
    desc = _abi.LitsInterDesc(N=n, H=h, W=w, C=1, n_slices=1, src_h=int(src_hw[0]), src_w=int(src_hw[1]), im_scale=1, lab_scale=1,
                              obj_label=1, training=0, seed=0, noise_scale=0.0, margin=1, step=0, band=1, max_clicks=2,
                              G=int(guide_channel), gaussian=0 if stddev is None else 1,
                              stddev=0.0 if stddev is None else float(stddev))
    guide = torch.empty((n, h, w, int(guide_channel)), dtype=torch.float32, device=sample_tab.device)
    with _timed_hbm("click_guide_list", guide, 1):
        check(_abi.lib().unetk_click_guide_list(ctypes.byref(desc), ptr(sample_tab), ptr(pts), ptr(cnt), k, ptr(guide),
                                                stream_ptr()), "click_guide_list")
    return guide


def lits_inter_center(slices, sample_tab, shape, status, im_scale=64):
    """The base field of the geodesic guide (unetk_lits_inter_center): f32 [N, (H + 1) // 2, (W + 1) // 2], the value
    lits_inter_batch(training=False) writes at [:, ::2, ::2, C // 2] with the table's flips ignored, bit for bit.  shape = (C, H,
    W); status collects bit 1; it is NOT read here.  Current stream."""
    _require_cuda(slices, sample_tab, status)
    assert slices.dtype in (torch.int16, torch.uint16) and slices.is_contiguous() and slices.dim() == 3
    assert status.dtype == torch.int32 and status.numel() >= 1
    n = _inter_tab(sample_tab)
    desc = lits_inter_desc(slices, n, shape, im_scale=im_scale)
    nbytes = int(_abi.lib().unetk_lits_inter_center_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("lits_inter_center: unsupported shape {} (C odd, <= 7) from {} x {} slices".format(
            tuple(shape), slices.shape[1], slices.shape[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=slices.device)
    base = torch.empty((n, (desc.H + 1) // 2, (desc.W + 1) // 2), dtype=torch.float32, device=slices.device)
    with _timed_hbm("lits_inter_center", base, 1):
        check(_abi.lib().unetk_lits_inter_center(ctypes.byref(desc), ptr(slices), ptr(sample_tab), ptr(base), ptr(status), ptr(ws),
                                                 nbytes, stream_ptr()), "lits_inter_center")
    return base


def click_geodesic_desc(n, out_hw, src_hw, guide_channel=2):
    """The descriptor of unetk_click_geodesic: it reads the geometry and G; the store's and the simulator's fields only have
    to be valid."""
    return _abi.LitsInterDesc(N=int(n), H=int(out_hw[0]), W=int(out_hw[1]), C=1, n_slices=1, src_h=int(src_hw[0]), src_w=int(src_hw[1]),
                              im_scale=1, lab_scale=1, obj_label=1, training=0, seed=0, noise_scale=0.0, margin=1, step=0, band=1,
                              max_clicks=2, G=int(guide_channel), gaussian=0, stddev=0.0)


def click_geodesic_path(out_hw, src_hw=(1, 1)):
    """Where unetk_click_geodesic keeps a grid of this output size: 0 unsupported, 1 LDS, 2 workspace."""
    return int(_abi.lib().unetk_click_geodesic_path(ctypes.byref(click_geodesic_desc(1, out_hw, src_hw))))


def click_geodesic(sample_tab, base, pts, cnt, out_hw, guide_channel=2, want_dist=False, status=None, src_hw=None,
                   want_sweeps=False):
    """sp_guide f32 [N, H, W, guide_channel] of --geodesic_guide (unetk_click_geodesic; include/unetk.h has the definition):
    base f32 [N, hh, hw] (lits_inter_center's, or any field), pts int32 [N, 2, K, 2] with K <= 64 and cnt int32 [N, 2] in the
    crop boxes and under the flips of sample_tab.  guide_channel 2: (fg, bg); 1: fg - bg.  want_dist: also the raw distances
    f32 [N, 2, hh, hw]; want_sweeps: also the int32 [N, 2] sweeps each solve ran.  status int32 [1] collects bit 3 (a solve hit
    its sweep bound); it is NOT read here (None: a word of its own).  src_hw: the store's slice extent, which clamps the
    table's crop sizes as every kernel on the table clamps them (None: 16384 x 16384).  Current stream."""
    _require_cuda(sample_tab, base, pts, cnt)
    n = _inter_tab(sample_tab)
    assert pts.dtype == torch.int32 and pts.dim() == 4 and pts.shape[0] == n and pts.shape[1] == 2 and pts.shape[3] == 2
    assert pts.is_contiguous() and cnt.dtype == torch.int32 and tuple(cnt.shape) == (n, 2) and cnt.is_contiguous()
    k = int(pts.shape[2])
    h, w = int(out_hw[0]), int(out_hw[1])
    hh, hw = (h + 1) // 2, (w + 1) // 2
    assert base.dtype == torch.float32 and tuple(base.shape) == (n, hh, hw) and base.is_contiguous()
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=sample_tab.device)
    assert status.dtype == torch.int32 and status.numel() >= 1
    desc = click_geodesic_desc(n, (h, w), src_hw if src_hw is not None else (1 << 14, 1 << 14), guide_channel)
    nbytes = int(_abi.lib().unetk_click_geodesic_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("click_geodesic: unsupported output {} x {} (the half-resolution grid holds at most 2^18 pixels)".format(h, w))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=sample_tab.device)
    guide = torch.empty((n, h, w, int(guide_channel)), dtype=torch.float32, device=sample_tab.device)
    dist = torch.empty((n, 2, hh, hw), dtype=torch.float32, device=sample_tab.device) if want_dist else None
    with _timed_hbm("click_geodesic", guide, 1):
        check(_abi.lib().unetk_click_geodesic(ctypes.byref(desc), ptr(sample_tab), ptr(base), ptr(pts), ptr(cnt), k, ptr(guide),
                                              ptr(dist) if want_dist else None, ptr(status), ptr(ws), nbytes, stream_ptr()),
              "click_geodesic")
    out = (guide,)
    if want_dist:
        out += (dist,)
    if want_sweeps:
        out += (ws[:n * 8].view(torch.int32).view(n, 2),)
    return out[0] if len(out) == 1 else out


def inter_click_desc(seg_slices, n, pred_hw, k, obj_label=1, lab_scale=64, vol_base=0, vol_depth=0):
    """The descriptor of unetk_inter_click (include/unetk.h)."""
    return _abi.InterClickDesc(N=int(n), H=int(pred_hw[0]), W=int(pred_hw[1]), n_slices=seg_slices.shape[0],
                               src_h=seg_slices.shape[1], src_w=seg_slices.shape[2], lab_scale=int(lab_scale),
                               obj_label=int(obj_label), K=int(k), vol_base=int(vol_base), vol_depth=int(vol_depth))


def inter_click_ws(desc, device):
    """A workspace of exactly the size unetk_inter_click asks for; raises where the query says unsupported."""
    nbytes = int(_abi.lib().unetk_inter_click_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("inter_click: unsupported ({} sessions, {} x {} slices, predictions {} x {}, K = {})".format(
            desc.N, desc.src_h, desc.src_w, desc.H, desc.W, desc.K))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def inter_click(seg_slices, rows, pred, pts, cnt, obj_label=1, lab_scale=64, vol=None, vol_base=0, pred_hw=None, table=None,
                ws=None):
    """One corrective click for every active session (unetk_inter_click; include/unetk.h has the semantics): rows int32 [N, 4]
    = (store slice, active, previous click y, x), pred uint8 [N, H, W] or None (all zeros; pred_hw then gives H, W), pts int32
    [N, 2, K, 2] / cnt int32 [N, 2] the click lists (appended to in place), vol uint8 [depth, src_h, src_w] or None the case's
    prediction volume starting at store slice vol_base.  Returns the int32 [N, 16] table.  Nothing is read back here.
    Current stream."""
    _require_cuda(seg_slices, rows, pts, cnt)
    assert seg_slices.dtype == torch.uint8 and seg_slices.dim() == 3 and seg_slices.is_contiguous()
    n = rows.shape[0]
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (n, _abi.INTER_ROW_COLS) and rows.is_contiguous()
    assert pts.dtype == torch.int32 and pts.dim() == 4 and pts.shape[0] == n and pts.shape[1] == 2 and pts.shape[3] == 2
    assert pts.is_contiguous() and cnt.dtype == torch.int32 and tuple(cnt.shape) == (n, 2) and cnt.is_contiguous()
    if pred is not None:
        assert pred.is_cuda and pred.dtype == torch.uint8 and pred.dim() == 3 and pred.shape[0] == n and pred.is_contiguous()
        pred_hw = pred.shape[1:]
    depth = 0
    if vol is not None:
        assert vol.is_cuda and vol.dtype == torch.uint8 and vol.is_contiguous() and tuple(vol.shape[1:]) == tuple(seg_slices.shape[1:])
        depth = vol.shape[0]
    desc = inter_click_desc(seg_slices, n, pred_hw, pts.shape[2], obj_label, lab_scale, vol_base, depth)
    if ws is None:
        ws = inter_click_ws(desc, seg_slices.device)
    if table is None:
        table = torch.empty((n, _abi.INTER_TAB_COLS), dtype=torch.int32, device=seg_slices.device)
    assert table.dtype == torch.int32 and tuple(table.shape) == (n, _abi.INTER_TAB_COLS) and table.is_contiguous()
    with _timed_hbm("inter_click", ws, 1):
        check(_abi.lib().unetk_inter_click(ctypes.byref(desc), ptr(seg_slices), ptr(rows), ptr(pred), ptr(vol), ptr(pts), ptr(cnt),
                                           ptr(table), ptr(ws), ws.numel(), stream_ptr()), "inter_click")
    return table


def lits3d_clicks_desc(seg_slices, n, shape, obj_label=1, clicks=(3, 10, 40, 5), lab_scale=64, guide_channel=2, stddev=None,
                       euclid_norm=1.0):
    """The descriptor of unetk_lits3d_clicks and unetk_click_guide3d (include/unetk.h): shape = (D, H, W), clicks = (margin,
    step, band, max_clicks) -- the reference's 3, 10, 40, 5 (input_pipeline_3d.py:492-503).  stddev None: the Euclidean
    guide divided by euclid_norm; (s_z, s_y, s_x): the Gaussian of --local_enhance."""
    d, h, w = (int(v) for v in shape)
    margin, step, band, max_clicks = (int(v) for v in clicks)
    sd = (0.0, 0.0, 0.0) if stddev is None else tuple(float(v) for v in stddev)
    assert len(sd) == 3
    return _abi.Lits3dClicksDesc(N=int(n), D=d, H=h, W=w, n_slices=seg_slices.shape[0], src_h=seg_slices.shape[1],
                                 src_w=seg_slices.shape[2], lab_scale=int(lab_scale), obj_label=int(obj_label), margin=margin,
                                 step=step, band=band, max_clicks=max_clicks, G=int(guide_channel),
                                 gaussian=0 if stddev is None else 1, stddev=(ctypes.c_float * 3)(*sd),
                                 euclid_norm=float(euclid_norm))


def lits3d_clicks(seg_slices, sample_tab, click_tab, shape, status, obj_label=1, clicks=(3, 10, 40, 5), lab_scale=64, neg_slices=None):
    """The simulated 3-D clicks of a batch (unetk_lits3d_clicks; include/unetk.h has the semantics) on the label patches
    `lits_patch3d` cuts for sample_tab int32 [N, 16], shape = (D, H, W); click_tab uint32-valued int32 [N, 12] = the samples'
    draws (data/lits_inter.draw_click_tab).  Returns pts int32 [N, 2, 4, 3] = (kind fg / bg, click, (z, y, x) in the crop; -1
    padding) and cnt int32 [N, 2].  status collects bit 2 (value 4); it is NOT read here.  Current stream.
    neg_slices: the `neg` plane of hard-negative training, uint8 of seg_slices' shape -> unetk_lits3d_clicks_neg: the
    background clicks of a row whose crop holds false positives are rank picks among them."""
    _require_cuda(seg_slices, sample_tab, click_tab, status)
    assert seg_slices.dtype == torch.uint8 and seg_slices.dim() == 3 and seg_slices.is_contiguous()
    if neg_slices is not None:
        _require_cuda(neg_slices)
        assert neg_slices.dtype == torch.uint8 and neg_slices.shape == seg_slices.shape and neg_slices.is_contiguous()
    n = _inter_tab(sample_tab)
    assert click_tab.dtype == torch.int32 and tuple(click_tab.shape) == (n, _abi.LITS_CLICK_TAB_COLS) and click_tab.is_contiguous()
    assert status.dtype == torch.int32 and status.numel() >= 1
    desc = lits3d_clicks_desc(seg_slices, n, shape, obj_label, clicks, lab_scale)
    nbytes = int(_abi.lib().unetk_lits3d_clicks_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("lits3d_clicks: unsupported parameters {} or depth {} on {} x {} slices".format(
            tuple(clicks), desc.D, seg_slices.shape[1], seg_slices.shape[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=seg_slices.device)
    pts = torch.empty((n, 2, _abi.LITS_MAX_CLICKS, 3), dtype=torch.int32, device=seg_slices.device)
    cnt = torch.empty((n, 2), dtype=torch.int32, device=seg_slices.device)
    with _timed_hbm("lits3d_clicks", ws, 1):
        if neg_slices is None:
            check(_abi.lib().unetk_lits3d_clicks(ctypes.byref(desc), ptr(seg_slices), ptr(sample_tab), ptr(click_tab), ptr(pts),
                                                 ptr(cnt), ptr(status), ptr(ws), nbytes, stream_ptr()), "lits3d_clicks")
        else:
            check(_abi.lib().unetk_lits3d_clicks_neg(ctypes.byref(desc), ptr(seg_slices), ptr(neg_slices), ptr(sample_tab),
                                                     ptr(click_tab), ptr(pts), ptr(cnt), ptr(status), ptr(ws), nbytes,
                                                     stream_ptr()), "lits3d_clicks_neg")
    return pts, cnt


def _click_guide3d_args(sample_tab, n, shape, src_hw, guide_channel, stddev, euclid_norm):
    """(descriptor, empty guide [n, D, H, W, guide_channel]) of unetk_click_guide3d and unetk_click_guide3d_list."""
    d, h, w = (int(v) for v in shape)
    if euclid_norm is None:
        euclid_norm = click_guide3d_norm(h)
    # the guide reads the geometry and its own fields; the store's and the simulator's only have to be valid
    desc = _abi.Lits3dClicksDesc(N=n, D=d, H=h, W=w, n_slices=1, src_h=int(src_hw[0]), src_w=int(src_hw[1]), lab_scale=1,
                                 obj_label=1, margin=1, step=0, band=1, max_clicks=2, G=int(guide_channel),
                                 gaussian=0 if stddev is None else 1,
                                 stddev=(ctypes.c_float * 3)(*((0.0, 0.0, 0.0) if stddev is None else tuple(float(v) for v in stddev))),
                                 euclid_norm=float(euclid_norm))
    return desc, torch.empty((n, d, h, w, int(guide_channel)), dtype=torch.float32, device=sample_tab.device)


def click_guide3d(sample_tab, pts, cnt, shape, src_hw, guide_channel=2, stddev=None, euclid_norm=None, rotate=False, warp=None,
                  grid=0):
    """sp_guide f32 [N, D, H, W, guide_channel] from 3-D clicks (unetk_click_guide3d): pts int32 [N, 2, 4, 3], cnt int32 [N, 2],
    in the crop boxes and under the three flips of sample_tab; shape = (D, H, W).  stddev None: the Euclidean distance to the
    nearest click divided by euclid_norm (default: float32(H * sqrt(2) * 0.8), input_pipeline_3d.py:372); (s_z, s_y, s_x):
    the Gaussian of --local_enhance.  guide_channel 2: (fg, bg); 1: fg - bg.  rotate: unetk_click_guide3d_rot, the guide of
    the patches `lits_patch3d(..., rotate=True)` cuts.  warp, grid: unetk_click_guide3d_warp, the guide of
    the patches `lits_patch3d(..., warp=warp, grid=grid)` cuts.  Current stream."""
    _require_cuda(sample_tab, pts, cnt)
    n = _inter_tab(sample_tab)
    assert pts.dtype == torch.int32 and tuple(pts.shape) == (n, 2, _abi.LITS_MAX_CLICKS, 3) and pts.is_contiguous()
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (n, 2) and cnt.is_contiguous()
    desc, guide = _click_guide3d_args(sample_tab, n, shape, src_hw, guide_channel, stddev, euclid_norm)
    name = "click_guide3d_warp" if warp is not None else "click_guide3d_rot" if rotate else "click_guide3d"
    lattice = () if warp is None else (ptr(warp), _warp_lattice(warp, grid, n, sample_tab.device))
    with _timed_hbm(name, guide, 1):
        check(getattr(_abi.lib(), "unetk_" + name)(ctypes.byref(desc), ptr(sample_tab), *lattice, ptr(pts), ptr(cnt), ptr(guide),
                                                   stream_ptr()), name)
    return guide


def click_guide3d_list(sample_tab, pts, cnt, shape, src_hw, guide_channel=2, stddev=None, euclid_norm=None):
    """click_guide3d for the rows of sample_tab from ONE pair of click lists in case coordinates (unetk_click_guide3d_list): pts
    int32 [2, K, 3] with K <= 64 = (kind, click, (z from the case's first slice, y, x)), cnt int32 [2].  Each row subtracts its
    crop box's origin; the same kernel: bit-equal to click_guide3d fed the clicks relative to the box.  Current stream."""
    _require_cuda(sample_tab, pts, cnt)
    n = _inter_tab(sample_tab)
    assert pts.dtype == torch.int32 and pts.dim() == 3 and pts.shape[0] == 2 and pts.shape[2] == 3 and pts.is_contiguous()
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (2,) and cnt.is_contiguous()
    desc, guide = _click_guide3d_args(sample_tab, n, shape, src_hw, guide_channel, stddev, euclid_norm)
    with _timed_hbm("click_guide3d_list", guide, 1):
        check(_abi.lib().unetk_click_guide3d_list(ctypes.byref(desc), ptr(sample_tab), ptr(pts), ptr(cnt), int(pts.shape[1]),
                                                  ptr(guide), stream_ptr()), "click_guide3d_list")
    return guide


SLICE_PRIOR_MODES = {"boundary": _abi.SLICE_PRIOR_BOUNDARY, "binary": _abi.SLICE_PRIOR_BINARY}


def slice_prior_field(seg_slices, sample_tab, pts, cnt, shape, obj_label=1, mode="boundary", whole=False, lab_scale=64):
    """The slice-prior field of every row of sample_tab int32 [N, 16] (unetk_slice_prior_field; include/unetk.h has the rule):
    (field int32 [N, src_h * src_w], z0 int32 [N]).  pts int32 [N, 2, 4, 3] / cnt int32 [N, 2]: the rows' own clicks
    (`lits3d_clicks`), or pts int32 [2, K, 3] / cnt int32 [2]: ONE pair of lists for all rows; z0 = the first foreground
    click's slice, read on the device.  whole=False: the box is the row's crop box, stored densely (pitch cw) at the start of
    its plane, z0 relative to the box; whole=True: the whole slice, z0 from the case's first slice.  mode "boundary": the
    exact squared Euclidean distance to the inner boundary of the object on that slice, -1 everywhere where there is none;
    "binary": the 0 / 1 mask.  Current stream; nothing is read back."""
    _require_cuda(seg_slices, sample_tab, pts, cnt)
    assert seg_slices.dtype == torch.uint8 and seg_slices.dim() == 3 and seg_slices.is_contiguous()
    n = _inter_tab(sample_tab)
    assert pts.dtype == torch.int32 and cnt.dtype == torch.int32 and pts.is_contiguous() and cnt.is_contiguous()
    if pts.dim() == 4:
        assert tuple(pts.shape) == (n, 2, _abi.LITS_MAX_CLICKS, 3) and tuple(cnt.shape) == (n, 2)
        k = 0
    else:
        assert pts.dim() == 3 and pts.shape[0] == 2 and pts.shape[2] == 3 and tuple(cnt.shape) == (2,)
        k = int(pts.shape[1])
    desc = lits3d_clicks_desc(seg_slices, n, shape, obj_label, lab_scale=lab_scale)
    nbytes = int(_abi.lib().unetk_slice_prior_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("slice_prior_field: unsupported slices of {} x {}".format(seg_slices.shape[1], seg_slices.shape[2]))
    binary = SLICE_PRIOR_MODES[mode] == _abi.SLICE_PRIOR_BINARY
    ws = None if binary else torch.empty(nbytes, dtype=torch.uint8, device=seg_slices.device)     # binary: the row pass alone
    field = torch.empty((n, seg_slices.shape[1] * seg_slices.shape[2]), dtype=torch.int32, device=seg_slices.device)
    z0 = torch.empty(n, dtype=torch.int32, device=seg_slices.device)
    with _timed_hbm("slice_prior_field", field, 1 if binary else 3):
        check(_abi.lib().unetk_slice_prior_field(ctypes.byref(desc), ptr(seg_slices), ptr(sample_tab), ptr(pts), ptr(cnt), k,
                                                 1 if whole else 0, SLICE_PRIOR_MODES[mode], ptr(field), ptr(z0),
                                                 ptr(ws), 0 if binary else nbytes, stream_ptr()),
              "slice_prior_field")
    return field, z0


def slice_prior_render(sample_tab, images, field, z0, shape, src_hw, mode="boundary", shared=False):
    """images f32 [N, D, H, W, 2] (unetk_slice_prior_render): channel 0 = images [N, D, H, W, 1] of `lits_patch3d` for the same
    table, bit for bit; channel 1 = the prior rendered from `slice_prior_field`'s (field, z0) in the rows' crop boxes and under
    their flips.  shared: ONE whole-slice field [1, src_h * src_w] and z0 [1] in case coordinates for all rows (a window table of
    one case).  Current stream."""
    _require_cuda(sample_tab, images, field, z0)
    n = _inter_tab(sample_tab)
    d, h, w = (int(v) for v in shape)
    plane = int(src_hw[0]) * int(src_hw[1])
    assert images.dtype == torch.float32 and tuple(images.shape) == (n, d, h, w, 1) and images.is_contiguous()
    assert field.dtype == torch.int32 and field.is_contiguous() and z0.dtype == torch.int32 and z0.is_contiguous()
    assert tuple(field.shape) == ((1 if shared else n), plane) and z0.numel() == (1 if shared else n), (tuple(field.shape), z0.shape)
    desc = _abi.Lits3dClicksDesc(N=n, D=d, H=h, W=w, n_slices=1, src_h=int(src_hw[0]), src_w=int(src_hw[1]), lab_scale=1,
                                 obj_label=1, margin=1, step=0, band=1, max_clicks=2, G=2, gaussian=0,
                                 stddev=(ctypes.c_float * 3)(0.0, 0.0, 0.0), euclid_norm=1.0)
    out = torch.empty((n, d, h, w, 2), dtype=torch.float32, device=images.device)
    with _timed_hbm("slice_prior_render", out, 1, images.numel() * 4):
        check(_abi.lib().unetk_slice_prior_render(ctypes.byref(desc), ptr(sample_tab), ptr(images), ptr(field), ptr(z0),
                                                  1 if shared else 0, SLICE_PRIOR_MODES[mode], ptr(out), stream_ptr()),
              "slice_prior_render")
    return out


def inter_click3d_desc(seg_slices, case_base, depth, k, obj_label=1, lab_scale=64, dist_cap=255):
    """The descriptor of unetk_inter_click3d (include/unetk.h)."""
    return _abi.InterClick3dDesc(case_base=int(case_base), depth=int(depth), n_slices=seg_slices.shape[0],
                                 src_h=seg_slices.shape[1], src_w=seg_slices.shape[2], lab_scale=int(lab_scale),
                                 obj_label=int(obj_label), K=int(k), dist_cap=int(dist_cap))


def inter_click3d_ws(desc, device):
    """A workspace of exactly the size unetk_inter_click3d asks for; raises where the query says unsupported."""
    nbytes = int(_abi.lib().unetk_inter_click3d_ws_bytes(ctypes.byref(desc)))
    if nbytes == 0:
        raise _abi.UnetkError("inter_click3d: unsupported (a case of {} x {} x {}, K = {}, dist_cap = {})".format(
            desc.depth, desc.src_h, desc.src_w, desc.K, desc.dist_cap))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def inter_click3d(seg_slices, case_base, depth, pred, prev, pts, cnt, obj_label=1, lab_scale=64, dist_cap=255, table=None, ws=None):
    """One corrective 3-D click for a case (unetk_inter_click3d; include/unetk.h has the semantics): the case is store slices
    [case_base, case_base + depth); pred uint8 [depth, src_h, src_w] or None (all zeros); prev = the previous click (z, y, x) or
    None; pts int32 [2, K, 3] / cnt int32 [2] the case's click lists in case coordinates (appended to in place).  Returns the
    int32 [20] table row.  Nothing is read back here.  Current stream."""
    _require_cuda(seg_slices, pts, cnt)
    assert seg_slices.dtype == torch.uint8 and seg_slices.dim() == 3 and seg_slices.is_contiguous()
    assert pts.dtype == torch.int32 and pts.dim() == 3 and pts.shape[0] == 2 and pts.shape[2] == 3 and pts.is_contiguous()
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (2,) and cnt.is_contiguous()
    if pred is not None:
        assert pred.is_cuda and pred.dtype == torch.uint8 and pred.is_contiguous()
        assert tuple(pred.shape) == (int(depth),) + tuple(seg_slices.shape[1:])
    desc = inter_click3d_desc(seg_slices, case_base, depth, pts.shape[1], obj_label, lab_scale, dist_cap)
    if ws is None:
        ws = inter_click3d_ws(desc, seg_slices.device)
    if table is None:
        table = torch.empty(_abi.INTER3D_TAB_COLS, dtype=torch.int32, device=seg_slices.device)
    assert table.dtype == torch.int32 and table.numel() == _abi.INTER3D_TAB_COLS and table.is_contiguous()
    pz, py, px = (-1, -1, -1) if prev is None else (int(v) for v in prev)
    with _timed_hbm("inter_click3d", ws, 1):
        check(_abi.lib().unetk_inter_click3d(ctypes.byref(desc), ptr(seg_slices), ptr(pred), pz, py, px, ptr(pts), ptr(cnt),
                                             ptr(table), ptr(ws), ws.numel(), stream_ptr()), "inter_click3d")
    return table


def click_guide3d_norm(im_height):
    """The divisor of the Euclidean 3-D guide, float32(im_height * sqrt(2) * 0.8) (input_pipeline_3d.py:372: a python float
    that TensorFlow converts to the guide's float32)."""
    import math
    import numpy as np
    return float(np.float32(int(im_height) * math.sqrt(2) * 0.8))


def adam_step(p, g, m, v, lr_t, beta1, beta2, eps, gscale=1.0, l2=0.0, decoupled_wd=0.0):
    with _timed_hbm("adam_step", p, 7):            # reads p, g, m, v; writes p, m, v
        check(_abi.lib().unetk_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr_t, beta1, beta2, eps, gscale, l2,
                                         decoupled_wd, stream_ptr()), "adam_step")
    bump_param_gen()


def momentum_step(p, g, acc, lr, mom, nesterov, gscale=1.0, l2=0.0):
    check(_abi.lib().unetk_momentum_step(ptr(p), ptr(g), ptr(acc), p.numel(), lr, mom, 1 if nesterov else 0, gscale,
                                         l2, stream_ptr()), "momentum_step")
    bump_param_gen()


def sumsq(p):
    out = torch.empty((1,), dtype=torch.float32, device=p.device)
    ws = WORKSPACE.get(8192, p.device)
    check(_abi.lib().unetk_sumsq(ptr(p), p.numel(), ptr(out), ptr(ws), 8192, stream_ptr()), "sumsq")
    return out


def png_unfilter(filtered, h, w, bit_depth, out, status):
    """filtered uint8 [n, h * (1 + w * bit_depth / 8)] (inflated PNG rows) -> out [n, h, w] (uint8, or int16 / uint16 storage
    for 16-bit samples) on the device; status int32[1] collects invalid filter types (unetk_png_unfilter)."""
    _require_cuda(filtered, out, status)
    n = filtered.shape[0]
    assert filtered.dtype == torch.uint8 and filtered.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (n, h, w)
    assert out.element_size() == bit_depth // 8 and filtered.shape[1] >= h * (1 + w * bit_depth // 8)
    check(_abi.lib().unetk_png_unfilter(ptr(filtered), filtered.stride(0), n, h, w, bit_depth, ptr(out), h * w, ptr(status),
                                        stream_ptr()), "png_unfilter")
    return out


def nan_watch(value, flag, step):
    """flag (int32[2], zeroed by the caller) becomes (1, step) at the first step whose `value` (a device scalar) is NaN."""
    _require_cuda(value, flag)
    assert value.dtype == torch.float32 and flag.dtype == torch.int32 and flag.numel() >= 2
    check(_abi.lib().unetk_nan_watch(ptr(value), ptr(flag), int(step), stream_ptr()), "nan_watch")


def guide_moments(guide, per_sample):
    """[groups, G + G*G]: E[g_i] and E[g_i g_j] of a (pooled) guide [N, H, W, G] per statistics group (GUNet --fix)."""
    _require_cuda(guide)
    guide = guide.to(torch.float32).contiguous()
    n, g = guide.shape[0], guide.shape[-1]
    hw = guide.numel() // (n * g)
    out = torch.empty((n if per_sample else 1, g + g * g), dtype=torch.float32, device=guide.device)
    check(_abi.lib().unetk_guide_moments(ptr(guide), n, hw, g, 1 if per_sample else 0, ptr(out), stream_ptr()), "guide_moments")
    return out


def norm_drop_pool(d, y, aff):
    """--use_se with --dropout: (sum_p m_p xhat_p, sum_p m_p) per (sample, channel), [2, N, C] (unetk_norm_drop_pool)."""
    d.storage = _storage_of(y)
    sums = torch.empty((2, d.N, d.C), dtype=torch.float32, device=y.device)
    check(_abi.lib().unetk_norm_drop_pool(ctypes.byref(d), ptr(y), ptr(aff[0]), ptr(aff[1]), ptr(sums), stream_ptr()),
          "norm_drop_pool")
    return sums


def norm_se_bwd_add_drop(d, y, dy, aff, e_mat, k1, k2):
    check(_abi.lib().unetk_norm_se_bwd_add_drop(ctypes.byref(d), ptr(y), ptr(dy), ptr(aff[0]), ptr(aff[1]), ptr(aff[2]),
                                                ptr(e_mat.contiguous()), ptr(k1.contiguous()), ptr(k2.contiguous()),
                                                stream_ptr()), "norm_se_bwd_add_drop")
    return dy


def norm_se_bwd_add(d, y, dy, aff, a_mat, k2):
    check(_abi.lib().unetk_norm_se_bwd_add(ctypes.byref(d), ptr(y), ptr(dy), ptr(aff[0]), ptr(aff[1]), ptr(aff[2]),
                                           ptr(a_mat.contiguous()), ptr(k2.contiguous()), stream_ptr()), "norm_se_bwd_add")
    return dy


# ----------------------------------------------------------------------------- autograd nodes
class NormSpec(object):
    """How a conv unit is normalised (the slim arg_scope state around slim.conv2d)."""

    def __init__(self, kind="batch_norm", eps=1e-3, decay=0.999, training=True, bf16=False):
        assert kind in ("batch_norm", "instance_norm", "none")   # "none" = --without_norm: conv + bias + ReLU
        self.kind, self.eps, self.decay, self.training = kind, eps, decay, training
        self.guide_leaky = False   # LGNet: leaky-ReLU on the guide branch before it is added
        self.guide_alpha = 0.2     # its slope (tf.nn.leaky_relu default); 0 = the ReLU of GUNet --fix
        self.guide_per_sample = False   # gw [N, g, C] / gb [N, C]: per-sample folded guide weights (--fix under instance norm)
        self.guide_post = False    # gb is the block [bias, slope for s > 0, slope for s <= 0, post-shift] x C (after_affine + --fix)
        self.dropout = None        # (keep_prob, seed): slim.dropout on the normalised value (GUNet --dropout), training only
        self.se = None             # GUNet --use_se: callable (pooled [N, C], context slice) -> gains [N, C] (torch graph)
        self.bf16 = precision_of(bf16)   # 0 fp32 | 1 UNETK_BF16 (bf16 operands, fp32 tensors) | 2 UNETK_BF16S (+ bf16 tensors)

    @property
    def per_sample(self):
        return self.kind == "instance_norm"


class Conv3x3NormRelu(_Op):
    """z = relu(norm(conv3x3(x, w)) [+ spatial guide modulation]) -- one slim.conv2d(x, C, 3) unit:
    conv without bias, slim.batch_norm / slim.instance_norm with optional centre (beta) and scale (gamma),
    ReLU (NetworksV2/UNet.py:41-56,79; GUNet.py:162-217 `modulated_conv_block`)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, moving_mean, moving_var, spec, out, guide, gw, gb, den=None, dilation=1, se_feat=None):
        _require_cuda(x, w)
        cin, cout = w.shape[2], w.shape[3]
        dilation = int(dilation or 1)
        if dilation != 1 and (bool(getattr(spec, "bf16", False)) or not conv_uses_mfma(cin, cout)):
            raise _abi.UnetkError("atrous conv (rate {}) needs the fp32 MFMA path (Cin % 16, Cout % 64)".format(dilation))
        if den is not None:
            den = den.contiguous()
        mfma = conv_uses_mfma(cin, cout)
        prec = precision_of(getattr(spec, "bf16", 0))
        bf16 = prec if conv_uses_bf16(cin, cout) else 0
        if prec == _abi.BF16S:
            # bf16 storage: the matrix kernels need 64-channel blocks on both sides; the first layer (small Cin, direct
            # kernel) reads the fp32 image and writes bf16
            if mfma and (cin % 64 or cout % 64):
                raise _abi.UnetkError("bf16 storage needs Cin % 64 == 0 and Cout % 64 == 0 (got {}->{})".format(cin, cout))
            bf16 = prec
        need_dx = ctx.needs_input_grad[0]
        if mfma:
            wp_f, wp_d = conv3x3_pack(w, want_dgrad=need_dx, bf16=bf16)
        else:
            wp_f, wp_d = w, None
            if need_dx:
                raise _abi.UnetkError("conv3x3 input gradient needs Cin%64==0 and Cout%16==0 "
                                      "(got {}->{})".format(cin, cout))
        plain = spec.kind == "none"
        se = getattr(spec, "se", None)
        use_batch_stats = (spec.training or spec.per_sample) and not plain
        if se is not None and (plain or den is not None):
            raise _abi.UnetkError("--use_se needs a normalised unit and no other density gain")
        # ---- inference fast path: the affine is known before the conv (moving statistics / --without_norm), so conv +
        # (scale, shift) + ReLU [+ the 2 x 2 max-pool the unit feeds] are ONE kernel and the raw output never exists
        fprec = precision_of(bf16)          # UNETK_BF16S: bf16 activations in and out (the first layer reads the fp32 image)
        if FUSE_EVAL and not spec.training and not use_batch_stats and se is None and den is None and guide is None \
                and gb is None and fprec in (_abi.FP32, _abi.BF16S) and dilation == 1:
            n_, h_, w_ = x.shape[0], x.shape[1], x.shape[2]
            z = out if out is not None else torch.empty((n_, h_, w_, cout), dtype=storage_dtype(fprec), device=x.device)
            fd = ConvDesc(n_, h_, w_, cin, cout, _pix_stride(x), _pix_stride(z), fprec, 1)
            want_pool = bool(getattr(ctx, "want_pool", False)) and POOL_FUSED
            with_pool = want_pool and _abi.lib().unetk_conv3x3_fwd_affine_ok(ctypes.byref(fd), 1) == 1
            if (with_pool or _abi.lib().unetk_conv3x3_fwd_affine_ok(ctypes.byref(fd), 0) == 1) and z.dtype == storage_dtype(fprec):
                nd = norm_desc((n_, h_, w_, cout), False, _pix_stride(z), 0, 0, 0)
                if plain:
                    sc, sh = torch.ones_like(beta), beta.detach().contiguous()
                else:
                    aff = norm_finalize(nd, None, 0, gamma, beta, spec.eps, spec.decay, False, moving_mean, moving_var, x.device)
                    sc, sh = aff[2], aff[3]
                pooled = torch.empty((n_, h_ // 2, w_ // 2, cout), dtype=z.dtype, device=x.device) if with_pool else None
                nws = _abi.lib().unetk_conv3x3_ws_bytes(ctypes.byref(fd))
                ws = WORKSPACE.get(nws, x.device) if nws else None
                with _timed("conv3x3_fwd_affine", 18.0 * n_ * h_ * w_ * cin * cout, "infer {}x{}x{} {}->{}", (n_, h_, w_, cin, cout),
                            by_kernel=True):
                    check(_abi.lib().unetk_conv3x3_fwd_affine(ctypes.byref(fd), ptr(x), ptr(wp_f), ptr(sc), ptr(sh), ptr(z),
                                                              ptr(pooled), cout, ptr(ws), nws, stream_ptr()), "conv3x3_fwd_affine")
                ctx.pooled = pooled
                return alias(z) if out is not None else z
        y, stats, rows = conv3x3_fwd(x, wp_f, cout, want_stats=use_batch_stats or se is not None, bf16=bf16, dilation=dilation)
        z = out if out is not None else torch.empty_like(y)
        g_ch = 0 if guide is None else guide.shape[-1]
        if g_ch:
            gw = gw.contiguous()
        if gb is not None:                  # without a guide: a bare per-channel shift after the gain (after_affine)
            gb = gb.contiguous()
        d = norm_desc(y.shape, spec.per_sample, _pix_stride(z), g_ch, cout if g_ch else 0, 0)
        if g_ch and getattr(spec, "guide_leaky", False):      # LGNet: u = t + leaky_relu(guide . gw + gb); --fix: ReLU
            alpha = float(getattr(spec, "guide_alpha", 0.2))
            d.guide_leaky = 1 if alpha == 0.2 else 2           # 1 = tf.nn.leaky_relu's default slope, 2 = guide_alpha
            d.guide_alpha = alpha
        if g_ch and getattr(spec, "guide_post", False):       # GUNet after_affine + --fix: gb = [bias, slope+, slope-, post-shift] rows
            d.guide_leaky = 3
        if getattr(spec, "guide_per_sample", False):
            d.guide_per_sample = 1
            d.gw_stride = cout
        drop = getattr(spec, "dropout", None)
        if drop is not None and spec.training:
            d.dropout_keep, d.dropout_seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF
            if den is None and (g_ch or gb is not None) and not d.guide_leaky:
                den = torch.ones((x.shape[0], cout), dtype=torch.float32, device=x.device)   # the backward's separate sum du
        if plain:
            # --without_norm (UNet.py:47-48): z = relu(y + bias); `beta` carries the conv bias
            d.affine_only = 1
            one, zero = torch.ones_like(beta), torch.zeros_like(beta)
            aff = torch.stack([zero, one, one, beta.detach()]).reshape(4, 1, cout).contiguous()
        else:
            aff = norm_finalize(d, stats, rows, gamma, beta, spec.eps, spec.decay, spec.training, moving_mean,
                                moving_var, y.device, y=y)
        se_graph = None
        if se is not None:
            # GUNet.py:192-201: gains = sigmoid(fc(relu(fc(concat(mean_hw(net), context))))).  mean_hw(net)[b, c] =
            # gamma * xhat_mean[b, c] + beta with xhat_mean from the per-sample means of the raw conv output (the same
            # statistic partials, reduced per sample); the tiny [N, C] graph below is ordinary torch autograd, run
            # backwards from inside this node's backward (the gains' gradient is only known there)
            m_mean = None
            if d.dropout_keep > 0:
                # --dropout as well (GUNet.py:189-201): the gate pools the DROPPED-OUT value, mean_hw(m (gamma xhat + beta)) =
                # gamma * mean(m xhat) + beta * mean(m): two per-sample sums of their own (unetk_norm_drop_pool)
                sums = norm_drop_pool(d, y, aff)
                xhat_mean, m_mean = (sums[0] / float(d.HW)).detach(), (sums[1] / float(d.HW)).detach()
            else:
                ps = norm_desc(y.shape, True)
                mean_b = norm_finalize(ps, stats, rows, None, None, spec.eps, 0.0, True, None, None, y.device)[0]    # [N, C]
                xhat_mean = ((mean_b - aff[0]) * aff[1]).detach()
            with torch.enable_grad():
                g_leaf = gamma.detach().requires_grad_(True) if gamma is not None else None
                b_leaf = beta.detach().requires_grad_(True) if beta is not None else None
                pooled = xhat_mean if g_leaf is None else xhat_mean * g_leaf
                if b_leaf is not None:
                    pooled = pooled + (b_leaf if m_mean is None else m_mean * b_leaf)
                pooled = pooled + torch.zeros_like(xhat_mean).requires_grad_(True) if not pooled.requires_grad else pooled
                pooled.retain_grad()
                # the context slice comes from the OUTER graph (the context MLP): inside, a detached leaf stands in for it
                # and its gradient is handed back as this node's gradient for `se_feat`
                f_leaf = se_feat.detach().requires_grad_(True) if se_feat is not None else None
                gains = se(pooled, f_leaf)
            den = gains.detach().contiguous()
            se_graph = (g_leaf, b_leaf, pooled, gains, xhat_mean, f_leaf, m_mean)
        ctx.pooled = None
        if getattr(ctx, "want_pool", False) and POOL_FUSED and se is None and den is None and g_ch == 0 and gb is None \
                and d.dropout_keep == 0 and y.shape[1] % 2 == 0 and y.shape[2] % 2 == 0:
            ctx.pooled = norm_apply_relu_pool(d, y, aff, z)        # Conv3x3NormReluPool: the pool rides on the apply pass
        else:
            norm_apply_relu(d, y, aff, z, guide, gw, gb, den)
        # a unit another conv unit may fuse its input gradient with (see conv3x3_dgrad): plain normalised units only
        simple = (not plain and se is None and den is None and g_ch == 0 and gb is None and d.dropout_keep == 0)
        if spec.training:
            src = getattr(x, "_unetk_unit", None)
            ctx.producer = src if (need_dx and src is not None and dilation == 1) else None
            ctx.simple = simple
            if getattr(ctx, "want_pool", False):
                ctx.unit_saved = (x, y, aff, guide, gw, gb, den)       # Conv3x3NormReluPool saves these together with its outputs
            else:
                ctx.save_for_backward(x, y, aff, guide, gw, gb, den)
            ctx.se_graph = se_graph
            ctx.wp_d = wp_d
            ctx.need_dx = need_dx
            ctx.bf16 = bf16
            ctx.dilation = dilation
            ctx.desc = d
            ctx.has = (gamma is not None, beta is not None)
            # gamma / beta of a unit with an SE gate also get gradient from the gate's graph: those stay with autograd
            ctx.sinks = (grad_sink(w, ctx), grad_sink(gamma, ctx) if se is None else None, grad_sink(beta, ctx) if se is None and not plain else None)
            ctx.w_dbg = w.detach() if DEBUG_CAPTURE is not None else None
            ctx.gb_dbg = (gamma, beta) if DEBUG_CAPTURE is not None else None
            ctx.z_dbg = z.detach() if DEBUG_CAPTURE is not None else None      # the forward's own ReLU mask, for the checkers
        zr = alias(z) if out is not None else z
        if spec.training and simple and out is None:
            zr._unetk_unit = (y, aff, spec.per_sample)
        return zr

    @staticmethod
    def backward(ctx, dz):
        return Conv3x3NormRelu._backward(ctx, dz)

    @staticmethod
    def _backward(ctx, dz, pool=None):
        """`pool` = (dp, dskip): the unit's activation fed max_pool2d and the skip connection (Conv3x3NormReluPool) and its
        gradient dz = dskip + route(dp) is formed inside the norm backward's two passes instead of being written first."""
        x, y, aff, guide, gw, gb, den = ctx.saved_tensors[:7]
        pre = None
        if pool is None:
            pre = FUSED_NBR.pop(dz.data_ptr(), None) if DEBUG_CAPTURE is None else None
            if pre is not None and not (ctx.simple and pre[0] == y.data_ptr() and pre[1] == tuple(dz.shape) and dz.is_contiguous()
                                        and pre[4] == dz._version):
                pre = None
            if dz.stride(3) != 1:
                dz = dz.contiguous()
            if dz.dtype != y.dtype:
                raise _abi.UnetkError("gradient dtype {} does not match the stored activations ({})".format(dz.dtype, y.dtype))
        dden = dfeat = None
        debug = DEBUG_CAPTURE is not None            # the checkers read the returned tensors
        sw, sg, sb = (None, None, None) if debug else (_take(ctx.sinks[0]), _take(ctx.sinks[1]), _take(ctx.sinks[2]))
        if pool is not None:
            dy, dgamma, dbeta = norm_relu_bwd_pool(ctx.desc, y, pool[1], pool[0], aff, ctx.has[0], ctx.has[1],
                                                   out_gamma=sg, out_beta=sb)
            dgw = dgb = None
        elif den is None:
            dy, dgamma, dbeta, dgw, dgb = norm_relu_bwd(ctx.desc, y, dz, aff, ctx.has[0], ctx.has[1], guide, gw, gb,
                                                        out_gamma=sg, out_beta=sb, pre=(pre[2], pre[3]) if pre else None)
        else:
            dy, dgamma, dbeta, dgw, dgb, dden = norm_relu_bwd(ctx.desc, y, dz, aff, ctx.has[0], ctx.has[1], guide, gw, gb,
                                                              den, out_gamma=sg, out_beta=sb)
        if getattr(ctx, "se_graph", None) is not None:
            g_leaf, b_leaf, pooled, gains, xhat_mean, f_leaf, m_mean = ctx.se_graph
            torch.autograd.backward(gains, dden)              # FC parameters accumulate here; pooled.grad = d loss / d pooled
            gp = pooled.grad
            dfeat = f_leaf.grad if f_leaf is not None else None
            if g_leaf is not None and g_leaf.grad is not None:
                dgamma = dgamma + g_leaf.grad if dgamma is not None else g_leaf.grad
            if b_leaf is not None and b_leaf.grad is not None:
                dbeta = dbeta + b_leaf.grad if dbeta is not None else b_leaf.grad
            if m_mean is not None:
                # with dropout the pooled value depends on y under either norm: dt gets m_p * E[b, c]; the statistics terms of
                # the (linear) norm backward follow from the forward's two sums: mean(m E) = E mean(m), mean(m E xhat) = E mean(m xhat)
                e_mat = gp / float(ctx.desc.HW)
                k1, k2 = e_mat * m_mean, e_mat * xhat_mean
                if not ctx.desc.per_sample:
                    k1, k2 = k1.mean(dim=0, keepdim=True), k2.mean(dim=0, keepdim=True)
                norm_se_bwd_add_drop(ctx.desc, y, dy, aff, e_mat, k1, k2)
            elif not ctx.desc.per_sample:                     # under instance norm the pooled value does not depend on y
                hw = float(ctx.desc.HW)
                a_mat = gp / hw
                k2 = (a_mat * xhat_mean).mean(dim=0, keepdim=True)
                a_mat = a_mat - a_mat.mean(dim=0, keepdim=True)
                norm_se_bwd_add(ctx.desc, y, dy, aff, a_mat, k2)
            dden = None                                       # the gains are internal to this node
            ctx.se_graph = None
        if ctx.desc.dropout_keep > 0 and den is not None and not ctx.needs_input_grad[11]:
            dden = None
        on_side = side_wgrad_on(ctx.bf16) and not debug and sw is not None and ctx.need_dx
        if not on_side:
            dw = conv3x3_wgrad(x, dy, bf16=ctx.bf16, dilation=ctx.dilation, out=sw)
        elif SIDE_WGRAD_FIRST:      # queued behind dy only: runs beside this unit's input gradient
            dw = _wgrad_on_side(x, dy, ctx.bf16, ctx.dilation, sw)
        dx = conv3x3_dgrad(dy, ctx.wp_d, x.shape[3], bf16=ctx.bf16, dilation=ctx.dilation,
                           producer=ctx.producer if DEBUG_CAPTURE is None else None) if ctx.need_dx else None
        if on_side and not SIDE_WGRAD_FIRST:      # behind the input gradient in issue order: beside the next unit's norm backward
            dw = _wgrad_on_side(x, dy, ctx.bf16, ctx.dilation, sw)
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.append(dict(x=x, y=y, dilation=ctx.dilation, z=ctx.z_dbg, gamma=ctx.gb_dbg[0], beta=ctx.gb_dbg[1], aff=aff, dz=dz, dy=dy, dw=dw,
                                      dx=dx, dgamma=dgamma, dbeta=dbeta, w=ctx.w_dbg, guide=guide, gw=gw, gb=gb,
                                      dgw=dgw, dgb=dgb, per_sample=bool(ctx.desc.per_sample), bf16=ctx.bf16, den=den,
                                      dden=dden, guide_leaky=bool(ctx.desc.guide_leaky), plain=bool(ctx.desc.affine_only)))
        return dx, _ret(dw, sw), _ret(dgamma, sg), _ret(dbeta, sb), None, None, None, None, None, dgw, dgb, dden, None, dfeat


POOL_FUSED = os.environ.get("UNETK_POOL_FUSED", "1") != "0"     # 0: separate pool-backward pass (measurement)


class Conv3x3NormReluPool(_Op):
    """(p, z) = (max_pool2d(z, 2, 2), z) with z = Conv3x3NormRelu(x, ...): the second conv of an encoder level, whose
    activation feeds the pool and -- through the concat buffer it was written into -- the skip connection
    (NetworksV2/UNet.py:79-81,93).  One node for conv unit + pool so that the backward gets BOTH gradients of z, dp and
    dskip, and never writes their sum: unetk_norm_relu_bwd_pool routes dp to each window's first maximum and adds dskip
    inside the norm backward's reduction and apply passes (the MaxPoolSkip node's pass over z / dz disappears).  Plain
    normalised units only (what UNet's encoder is); anything else takes the two separate passes."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, moving_mean, moving_var, spec, out):
        ctx.want_pool = True
        z = Conv3x3NormRelu.forward(ctx, x, w, gamma, beta, moving_mean, moving_var, spec, out, None, None, None)
        p = ctx.pooled if ctx.pooled is not None else maxpool2_fwd(z)
        ctx.pooled = None
        if spec.training:
            # the node's own outputs go through save_for_backward like its inputs (a plain attribute would tie
            # p -> grad_fn -> ctx -> p into a cycle that only a backward run breaks); both are alive anyway: z is the skip
            # inside the concat buffer, p the next unit's input
            ctx.save_for_backward(*(ctx.unit_saved + (z, p)))
            ctx.unit_saved = None
        return p, z

    @staticmethod
    def backward(ctx, dp, dskip):
        z, p = ctx.saved_tensors[7:9]
        if dskip is not None and dskip.stride(3) != 1:
            dskip = dskip.contiguous()
        plain_unit = ctx.saved_tensors[3] is None and ctx.saved_tensors[5] is None and ctx.saved_tensors[6] is None \
            and ctx.desc.dropout_keep == 0 and getattr(ctx, "se_graph", None) is None
        if POOL_FUSED and DEBUG_CAPTURE is None and plain_unit and dp is not None and dskip is not None \
                and dp.dtype == z.dtype and dskip.dtype == z.dtype:
            return Conv3x3NormRelu._backward(ctx, None, pool=(dp.contiguous(), dskip))[:8]
        dz = dskip if dp is None else maxpool2_bwd(z, p, dp, dskip)
        return Conv3x3NormRelu._backward(ctx, dz)[:8]


class FullyConnected(_Op):
    """y = dropout(act(x . w + b)), act = identity (relu 0 / False), ReLU (1 / True) or sigmoid (2: the SE gate,
    GUNet.py:199) -- one slim.fully_connected (+ slim.dropout) of GUNet's context MLP
    (NetworksV2/Backbone/slim_nets.py:43-56; GUNet.py:50-60).  w is TF's [in, out].  keep_prob None = no dropout;
    the mask (0 or 1/keep_prob per element, counter RNG keyed by `seed`) is kept for the backward."""

    @staticmethod
    def forward(ctx, x, w, b, relu, keep_prob, seed):
        _require_cuda(x, w)
        x = x.contiguous()
        bsz, k = x.shape
        n = w.shape[1]
        assert w.shape[0] == k and w.is_contiguous()
        y = torch.empty((bsz, n), dtype=torch.float32, device=x.device)
        mask = torch.empty_like(y) if keep_prob is not None else None
        check(_abi.lib().unetk_fc_fwd(ptr(x), ptr(w), ptr(b), ptr(y), ptr(mask), bsz, k, n, int(relu or 0),
                                      float(keep_prob) if keep_prob is not None else 1.0, int(seed) & 0xFFFFFFFF,
                                      stream_ptr()), "fc_fwd")
        ctx.save_for_backward(x, w, y, mask)
        ctx.relu = relu
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, mask = ctx.saved_tensors
        dy = dy.contiguous()
        bsz, k = x.shape
        n = w.shape[1]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty((n,), dtype=torch.float32, device=x.device) if ctx.has_b else None
        ws = torch.empty_like(y)
        check(_abi.lib().unetk_fc_bwd(ptr(x), ptr(w), ptr(y), ptr(mask), ptr(dy), ptr(dx), ptr(dw), ptr(db), ptr(ws), bsz, k,
                                      n, int(ctx.relu or 0), stream_ptr()), "fc_bwd")
        return dx, dw, db, None, None, None


class Conv1d(_Op):
    """y = relu(conv1d(x, w) + b): slim.conv1d(x, C, k) with slim's defaults (stride 1, SAME, bias, ReLU) -- the layers of
    GUNet's 1-D VGG context models (NetworksV2/Backbone/slim_nets.py:60-144).  x [B, L, Cin], w TF [k, Cin, Cout]."""

    @staticmethod
    def forward(ctx, x, w, b, relu=True):
        _require_cuda(x, w)
        x = x.contiguous()
        bsz, length, cin = x.shape
        k, cin_w, cout = w.shape
        assert cin_w == cin and w.is_contiguous() and k in (1, 3)
        y = torch.empty((bsz, length, cout), dtype=torch.float32, device=x.device)
        check(_abi.lib().unetk_conv1d_fwd(ptr(x), ptr(w), ptr(b), ptr(y), bsz, length, cin, cout, k, 1 if relu else 0,
                                          stream_ptr()), "conv1d_fwd")
        ctx.save_for_backward(x, w, y)
        ctx.relu, ctx.has_b = bool(relu), b is not None
        ctx.sinks = (grad_sink(w, ctx), grad_sink(b, ctx))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        bsz, length, cin = x.shape
        k, _, cout = w.shape
        sw, sb = _take(ctx.sinks[0]), _take(ctx.sinks[1])
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = sw if sw is not None else torch.empty_like(w)
        db = (sb if sb is not None else torch.empty((cout,), dtype=torch.float32, device=x.device)) if ctx.has_b else None
        ws = torch.empty_like(y)
        check(_abi.lib().unetk_conv1d_bwd(ptr(x), ptr(w), ptr(y), ptr(dy), ptr(dx), ptr(dw), ptr(db), ptr(ws), bsz, length,
                                          cin, cout, k, 1 if ctx.relu else 0, stream_ptr()), "conv1d_bwd")
        return dx, _ret(dw, sw), (_ret(db, sb) if ctx.has_b else None), None


class MaxPool1d(_Op):
    """tf.layers.max_pooling1d(x, 2, 2, padding="same") on [B, L, C] (slim_nets.py:73 ...): Lo = ceil(L / 2)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        x = x.contiguous()
        bsz, length, c = x.shape
        y = torch.empty((bsz, (length + 1) // 2, c), dtype=torch.float32, device=x.device)
        check(_abi.lib().unetk_maxpool1d_fwd(ptr(x), ptr(y), bsz, length, c, stream_ptr()), "maxpool1d_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        bsz, length, c = x.shape
        dx = torch.empty_like(x)
        check(_abi.lib().unetk_maxpool1d_bwd(ptr(x), ptr(dy.contiguous()), ptr(dx), bsz, length, c, stream_ptr()),
              "maxpool1d_bwd")
        return dx


class SpatialMean(_Op):
    """tf.reduce_mean(x, axis=(1, 2)) on NHWC (GUNet.py:108, the conv context subnet)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        x = x.contiguous()
        n, c = x.shape[0], x.shape[-1]
        hw = x.numel() // (n * c)
        y = torch.empty((n, c), dtype=torch.float32, device=x.device)
        check(_abi.lib().unetk_spatial_mean_fwd(ptr(x), ptr(y), n, hw, c, stream_ptr()), "spatial_mean_fwd")
        ctx.shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c = ctx.shape[0], ctx.shape[-1]
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        check(_abi.lib().unetk_spatial_mean_bwd(ptr(dy.contiguous()), ptr(dx), n, dx.numel() // (n * c), c, stream_ptr()),
              "spatial_mean_bwd")
        return dx


class Conv3dNormRelu(_Op):
    """z = relu(norm(conv3d(x, w))) -- one slim.conv3d unit of UNet3D (UNet3D.py:108-121,153,165): kernel
    (1,3,3) or (3,3,3), stride 1 / (1,2,2) / (2,2,2), SAME, no bias, instance or batch norm, ReLU."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, moving_mean, moving_var, spec, stride, out, precision=0):
        """precision: UNETK_FP32, or UNETK_BF16 (--compute_dtype bf16c) -- applied when the layer meets the rule of
        conv3d_bf16_ok, else the layer runs exact fp32."""
        _require_cuda(x, w)
        kd, cin, cout = w.shape[0], w.shape[3], w.shape[4]
        mfma = conv_uses_mfma(cin, cout)
        need_dx = ctx.needs_input_grad[0]
        live8 = getattr(w, "unetk_live8", None)      # set on channel-padded filters by PaddedParamStore
        d = conv3d_desc(x.shape, cout, kd, stride, x_stride=_pix_stride_nd(x), live8=live8)
        prec = conv3d_precision(d, precision)
        if prec:
            wp_f, wp_d = conv3d_pack(w, want_dgrad=need_dx, precision=prec)
        elif mfma:
            wp_f, wp_d = conv3d_pack(w, want_dgrad=need_dx)
        else:
            if kd != 1 or need_dx:
                raise _abi.UnetkError("conv3d with Cin={} Cout={} needs the MFMA path (Cin%16, Cout%32)".format(cin, cout))
            wp_f, wp_d = w, None
        plain = spec.kind == "none"                # --without_norm: z = relu(y + bias); `beta` carries the conv bias
        use_batch_stats = (spec.training or spec.per_sample) and not plain
        y, stats, rows = conv3d_fwd(x, wp_f, d, want_stats=use_batch_stats, precision=prec)
        z = out if out is not None else torch.empty_like(y)
        nd = norm_desc(y.shape, spec.per_sample, _pix_stride_nd(z))
        if plain:
            nd.affine_only = 1
            one, zero = torch.ones_like(beta), torch.zeros_like(beta)
            aff = torch.stack([zero, one, one, beta.detach()]).reshape(4, 1, cout).contiguous()
        else:
            aff = norm_finalize(nd, stats, rows, gamma, beta, spec.eps, spec.decay, spec.training, moving_mean, moving_var,
                                y.device, y=y)
        norm_apply_relu(nd, y, aff, z)
        if spec.training:
            ctx.save_for_backward(x, y, aff)
            ctx.wp_d, ctx.need_dx, ctx.d, ctx.nd, ctx.live8, ctx.prec = wp_d, need_dx, d, nd, live8, prec
            ctx.has = (gamma is not None, beta is not None)
            ctx.sinks = (grad_sink(w, ctx), grad_sink(gamma, ctx), grad_sink(beta, ctx) if not plain else None)
            ctx.dbg = (w.detach(), gamma, beta, stride, z.detach()) if DEBUG_CAPTURE is not None else None
        return alias(z) if out is not None else z

    @staticmethod
    def backward(ctx, dz):
        x, y, aff = ctx.saved_tensors
        if dz.stride(-1) != 1:
            dz = dz.contiguous()
        debug = DEBUG_CAPTURE is not None
        sw, sg, sb = (None, None, None) if debug else (_take(ctx.sinks[0]), _take(ctx.sinks[1]), _take(ctx.sinks[2]))
        dy, dgamma, dbeta, _, _ = norm_relu_bwd_nd(ctx.nd, y, dz, aff, ctx.has[0], ctx.has[1], out_gamma=sg, out_beta=sb)
        voxels = dy.numel() // dy.shape[-1]
        on_side = (not debug) and sw is not None and ctx.need_dx and 0 < voxels <= SIDE_WGRAD3D_VOXELS and not _Side.paused
        prec = ctx.prec
        if not on_side:
            dw = conv3d_wgrad(x, dy, ctx.d, out=sw, precision=prec)
        elif SIDE_WGRAD3D_FIRST:
            dw = _wgrad3d_on_side(x, dy, ctx.d, sw, prec)      # queued behind dy only: runs BESIDE this layer's input gradient
        dense = conv3d_desc(x.shape, ctx.d.Cout, ctx.d.kd, (ctx.d.sd, ctx.d.shw, ctx.d.shw), live8=ctx.live8)   # dx is dense
        dx = conv3d_dgrad(dy, ctx.wp_d, dense, precision=prec) if ctx.need_dx else None
        if on_side and not SIDE_WGRAD3D_FIRST:
            dw = _wgrad3d_on_side(x, dy, ctx.d, sw, prec)      # queued behind the input gradient: runs beside the NEXT unit's norm backward
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.append(dict(kind="conv3d", x=x, y=y, w=ctx.dbg[0], gamma=ctx.dbg[1], beta=ctx.dbg[2],
                                      stride=ctx.dbg[3], z=ctx.dbg[4], dz=dz, dy=dy, dw=dw, dx=dx, dgamma=dgamma, dbeta=dbeta,
                                      per_sample=bool(ctx.nd.per_sample), plain=bool(ctx.nd.affine_only)))
        return dx, _ret(dw, sw), _ret(dgamma, sg), _ret(dbeta, sb), None, None, None, None, None, None


class Deconv3dConcat(_Op):
    """cat = concat(skip, relu(conv3d_transpose(x, w, kernel == stride))) -- UNet3D.py:161-163 (no bias);
    `skip` already lives in cat[..., :C], the kernel fills cat[..., C:]."""

    @staticmethod
    def forward(ctx, x, w, skip, cat, precision=0):
        """precision: UNETK_FP32, or UNETK_BF16 (bf16 matrix-core operands; Cin % 32 == 0 and Cout % 32 == 0, else fp32)."""
        _require_cuda(x, w, cat)
        kd, cout = w.shape[0], w.shape[3]
        cin = w.shape[4]
        coff = cat.shape[-1] - cout
        assert skip.data_ptr() == cat.data_ptr() and skip.shape[-1] == coff
        prec = _abi.BF16 if int(precision or 0) == _abi.BF16 and cin % 32 == 0 and cout % 32 == 0 else _abi.FP32
        wp_f, wp_d = deconv3d_pack(w, precision=prec)
        deconv3d_fwd(x, wp_f, None, cat, coff, cout, kd, precision=prec)
        ctx.save_for_backward(x, cat)
        ctx.wp_d, ctx.cout, ctx.coff, ctx.kd, ctx.prec = wp_d, cout, coff, kd, prec
        ctx.sink = grad_sink(w, ctx)
        ctx.w_dbg = w.detach() if DEBUG_CAPTURE is not None else None
        return alias(cat)

    @staticmethod
    def backward(ctx, dcat):
        x, cat = ctx.saved_tensors
        dcat = dcat.contiguous()
        sw = None if DEBUG_CAPTURE is not None else _take(ctx.sink)
        dx, dw, _ = deconv3d_bwd(x, ctx.wp_d, cat, dcat, ctx.coff, ctx.cout, ctx.kd, want_dbias=False, out_w=sw,
                                 precision=ctx.prec)
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.append(dict(kind="deconv3d", x=x, w=ctx.w_dbg, cat=cat.clone(), dcat=dcat, dx=dx, dw=dw,
                                      coff=ctx.coff, kd=ctx.kd))
        return dx, _ret(dw, sw), dcat[..., :ctx.coff], None, None


class MaxPool2x2(_Op):
    @staticmethod
    def forward(ctx, x):
        p = maxpool2_fwd(x)
        ctx.save_for_backward(x, p)
        return p

    @staticmethod
    def backward(ctx, dp):
        x, p = ctx.saved_tensors
        return maxpool2_bwd(x, p, dp)


class MaxPoolSkip(_Op):
    """(p, skip) = (max_pool2d(x), x): the encoder activation feeds both the pool and the skip connection
    (UNet.py:80-81,93).  Returning the skip from the same node lets the backward sum the two gradients inside the pool
    backward kernel (dx = route(dp) + dskip, dskip read in place from the concat buffer's gradient) instead of a
    separate elementwise pass."""

    @staticmethod
    def forward(ctx, x):
        p = maxpool2_fwd(x)
        ctx.save_for_backward(x, p)
        return p, alias(x)

    @staticmethod
    def backward(ctx, dp, dskip):
        x, p = ctx.saved_tensors
        if dskip is not None and dskip.stride(3) != 1:
            dskip = dskip.contiguous()
        if dp is None:
            return dskip
        return maxpool2_bwd(x, p, dp, dskip)


class DeconvConcat(_Op):
    """cat = concat(skip, relu(conv2d_transpose(x, w, k=2, s=2) + b)); `skip` already lives in
    cat[..., :C] (the encoder wrote it there), the kernel fills cat[..., C:] -- zero-copy concat."""

    @staticmethod
    def forward(ctx, x, w, b, skip, cat, bf16=False):
        _require_cuda(x, w, b, cat)
        cout = w.shape[2]
        coff = cat.shape[3] - cout
        assert skip.data_ptr() == cat.data_ptr() and skip.shape[3] == coff
        bf16 = precision_of(bf16) if conv_uses_bf16(w.shape[3], cout) else 0
        if x.dtype == torch.bfloat16 and (bf16 != _abi.BF16S or w.shape[3] % 64 or cout % 64):
            raise _abi.UnetkError("bf16 storage needs Cin % 64 == 0 and Cout % 64 == 0 in the transposed conv")
        wp_f, wp_d = deconv2x2_pack(w, bf16)
        deconv2x2_fwd(x, wp_f, b, cat, coff, cout, bf16)
        ctx.save_for_backward(x, cat)
        ctx.wp_d = wp_d
        ctx.bf16 = bf16
        ctx.cout, ctx.coff = cout, coff
        ctx.has_b = b is not None            # SmallUNet's conv2d_transpose has biases_initializer=None
        ctx.sinks = (grad_sink(w, ctx), grad_sink(b, ctx))
        ctx.wb_dbg = (w.detach(), b.detach() if b is not None else None) if DEBUG_CAPTURE is not None else None
        return alias(cat)

    @staticmethod
    def backward(ctx, dcat):
        x, cat = ctx.saved_tensors
        dcat = dcat.contiguous()
        sw, sb = (None, None) if DEBUG_CAPTURE is not None else (_take(ctx.sinks[0]), _take(ctx.sinks[1]))
        dx, dw, db = deconv2x2_bwd(x, ctx.wp_d, cat, dcat, ctx.coff, ctx.cout, ctx.bf16, out_w=sw, out_b=sb)
        dskip = dcat[..., :ctx.coff]
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.append(dict(kind="deconv", x=x, w=ctx.wb_dbg[0], b=ctx.wb_dbg[1], cat=cat.clone(),
                                      dcat=dcat, dx=dx, dw=dw, db=db, coff=ctx.coff, bf16=ctx.bf16))
        return dx, _ret(dw, sw), (_ret(db, sb) if ctx.has_b else None), dskip, None, None


class DeconvConcatFront(_Op):
    """cat = concat(relu(conv2d_transpose(x, w, k=2, s=2) [+ b]), skip_a, skip_b) -- InterUNet's decoder (InterUNet.py:150-155:
    the up-sampled tensor FIRST, then the skips of the two encoders).  The skips already live in cat[..., C:] (their
    encoders wrote them there); the kernel fills cat[..., :C]."""

    @staticmethod
    def forward(ctx, x, w, b, skip_a, skip_b, cat):
        _require_cuda(x, w, cat)
        cout = w.shape[2]
        ca, cb = skip_a.shape[3], skip_b.shape[3]
        assert cat.shape[3] == cout + ca + cb
        assert skip_a.data_ptr() == cat.data_ptr() + 4 * cout and skip_b.data_ptr() == cat.data_ptr() + 4 * (cout + ca)
        wp_f, wp_d = deconv2x2_pack(w, False)
        deconv2x2_fwd(x, wp_f, b, cat, 0, cout, False)
        ctx.save_for_backward(x, cat)
        ctx.wp_d, ctx.cout, ctx.ca, ctx.has_b = wp_d, cout, ca, b is not None
        ctx.wb_dbg = (w.detach(), b.detach() if b is not None else None) if DEBUG_CAPTURE is not None else None
        return alias(cat)

    @staticmethod
    def backward(ctx, dcat):
        x, cat = ctx.saved_tensors
        dcat = dcat.contiguous()
        dx, dw, db = deconv2x2_bwd(x, ctx.wp_d, cat, dcat, 0, ctx.cout, False)
        if DEBUG_CAPTURE is not None:
            DEBUG_CAPTURE.append(dict(kind="deconv", x=x, w=ctx.wb_dbg[0], b=ctx.wb_dbg[1], cat=cat.clone(), dcat=dcat, dx=dx,
                                      dw=dw, db=db, coff=0, bf16=False))
        c0, c1 = ctx.cout, ctx.cout + ctx.ca
        return dx, dw, (db if ctx.has_b else None), dcat[..., c0:c1], dcat[..., c1:], None


class HeadLoss(_Op):
    """(xent, dice) = loss head over logits = z @ w + b; also returns logits / probs / metric sums
    as non-differentiable outputs."""

    @staticmethod
    def forward(ctx, z, w, b, labels, pixel_w, desc, want_probs):
        # undefined gradients stay None: autograd otherwise zero-fills a [N, H, W, classes] tensor per step for each of the
        # non-differentiable outputs (logits, probabilities: 2 x 25 MB at the headline shape) only to hand it to backward
        ctx.set_materialize_grads(False)
        w2 = w.reshape(desc.C, desc.ncls)
        logits, probs, result, ws = head_fwd(desc, z, w2, b, labels, pixel_w, want_probs)
        ctx.save_for_backward(z, w2, labels, pixel_w, logits, result, ws)
        ctx.desc = desc
        ctx.w_shape = w.shape
        ctx.sinks = (grad_sink(w, ctx), grad_sink(b, ctx))
        xent = result[0:1].reshape(())
        dice = result[1:2].reshape(())
        outs = (xent.clone(), dice.clone(), logits, probs if probs is not None else logits.new_empty(0), result)
        ctx.mark_non_differentiable(outs[2], outs[3], outs[4])
        return outs

    @staticmethod
    def backward(ctx, gx, gd, _gl, _gp, _gr):
        z, w2, labels, pixel_w, logits, result, ws = ctx.saved_tensors
        zero = torch.zeros((), dtype=torch.float32, device=z.device)
        scales = torch.stack([gx if gx is not None else zero, gd if gd is not None else zero]).to(torch.float32)
        sw, sb = _take(ctx.sinks[0]), _take(ctx.sinks[1])
        dz, dw, db = head_bwd(ctx.desc, z, w2, labels, pixel_w, logits, result, ws,
                              1.0 if gx is not None else 0.0, 1.0 if gd is not None else 0.0, scales,
                              out_w=sw.reshape(ctx.desc.C, ctx.desc.ncls) if sw is not None else None, out_b=sb)
        return dz, _ret(dw.reshape(ctx.w_shape), sw), _ret(db, sb), None, None, None, None
