"""Guarded device buffers for the edge tests of the kernels (test_gpu_guard_bands.py).

Every tensor a kernel sees is a view inside one larger flat allocation: a head guard, the payload (a pixel-strided channel
slice, the same kind of view as a concat buffer's half) and a tail guard, each guard at least 256 KiB and at least as large as
the payload, so that an overrun by a whole extra tile lands inside the allocation and is seen instead of faulting.

  Output:    everything outside the view holds a signalling-NaN sentinel (0x7FBADBAD fp32, 0x7FA5 bf16); after the call the
             bytes outside the view are compared bit for bit with the snapshot, and sentinels left INSIDE the view are the
             elements the kernel never wrote.
  Input:     the view holds the data, everything else a large finite poison (1e30): an over-fetch that is masked stays
             harmless, one that reaches the contraction shows up as a huge error.  The whole allocation must stay bit-equal.
  Workspace: exactly the queried number of bytes at an offset = 16 (mod 256) -- as aligned as the ABI promises and no more --
             followed by a sentinel guard.
"""
import torch

GUARD_MIN_BYTES = 256 << 10
SENTINEL = {torch.float32: 0x7FBADBAD, torch.bfloat16: 0x7FA5}
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
POISON = 1e30


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Guarded(object):
    """A [..., C] view with pixel stride `pixel_stride` (elements) at channel offset `coff` inside a guarded flat buffer."""

    def __init__(self, shape, dtype=torch.float32, pixel_stride=None, coff=0, fill=None, device="cuda"):
        shape = tuple(int(s) for s in shape)
        c = shape[-1]
        ps = c if pixel_stride is None else int(pixel_stride)
        assert 0 <= coff and coff + c <= ps
        esize = torch.empty((), dtype=dtype).element_size()
        npix = _numel(shape[:-1])
        payload = npix * ps
        guard = max(GUARD_MIN_BYTES // esize, payload)
        guard = (guard + 127) // 128 * 128               # 256-byte multiple: the view keeps the allocation's alignment
        self.shape, self.dtype, self.ps, self.coff, self.guard, self.payload = shape, dtype, ps, coff, guard, payload
        self.flat = torch.empty(2 * guard + payload, dtype=dtype, device=device)
        strides, acc = [1], ps
        for s in reversed(shape[:-1]):
            strides.insert(0, acc)
            acc *= s
        self.strides = tuple(strides)
        self.view = self.flat.as_strided(shape, self.strides, guard + coff)
        self.mask = torch.zeros(self.flat.numel(), dtype=torch.bool, device=device)
        self.mask.as_strided(shape, self.strides, guard + coff).fill_(True)
        if fill is None:                                  # an output: sentinel everywhere
            self.bits().fill_(SENTINEL[dtype])
        else:                                             # an input: finite poison around the data
            self.flat.fill_(POISON)
            self.view.copy_(fill)
        self.snap = self.flat.clone()

    def bits(self, t=None):
        return (self.flat if t is None else t).view(_BITS[self.dtype])

    def reset(self):
        self.flat.copy_(self.snap)

    def changed_outside(self):
        """Number of elements outside the view whose bits differ from the snapshot (guards and neighbour channels)."""
        return int((self.bits() != self.bits(self.snap))[~self.mask].sum())

    def changed_anywhere(self):
        return int((self.bits() != self.bits(self.snap)).sum())

    def check_untouched(self):
        return self.changed_outside() == 0

    def unwritten(self):
        """Sentinel patterns left inside the view."""
        return int((self.bits() == SENTINEL[self.dtype])[self.mask].sum())

    def ptr(self):
        return self.view.data_ptr()


def guarded(shape, dtype=torch.float32, pixel_stride=None, coff=0):
    """An output buffer (see the module docstring)."""
    return Guarded(shape, dtype, pixel_stride, coff)


def guarded_input(data, pixel_stride=None, coff=0, dtype=None):
    """An input buffer holding `data` (a device tensor [..., C]) in a poisoned guarded allocation."""
    dtype = dtype or data.dtype
    return Guarded(data.shape, dtype, pixel_stride, coff, fill=data.to(dtype), device=data.device)


class GuardedWorkspace(object):
    """`nbytes` of scratch at an offset = 16 (mod 256), followed by a sentinel guard.  nbytes == 0 still hands out a valid
    pointer (an entry point that wants a non-NULL ws of a zero-size query gets one; any byte it writes is in the guard)."""

    def __init__(self, nbytes, device="cuda"):
        self.nbytes = int(nbytes)
        guard = max(GUARD_MIN_BYTES, self.nbytes)
        self.off = 256 + 16
        size = (self.off + self.nbytes + guard + 256 + 3) // 4 * 4
        self.buf = torch.empty(size, dtype=torch.uint8, device=device)
        self.off += (-self.buf.data_ptr()) % 256
        self.buf.view(torch.int32).fill_(SENTINEL[torch.float32])
        self.snap = self.buf.clone()

    def fill(self, byte):
        self.buf[self.off:self.off + self.nbytes].fill_(byte)

    def ptr(self):
        return self.buf.data_ptr() + self.off

    def guard_intact(self):
        """The bytes before and after [off, off + nbytes) are as they were."""
        outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        outside[self.off:self.off + self.nbytes] = False
        return bool(torch.equal(self.buf[outside], self.snap[outside]))
