"""Guarded device buffers for the tests of the device-pointer (_dev) entry points.

The host forms lay every array out in one staging arena, 256-byte aligned and rounded up to
256 bytes, and copy back only the valid prefix, so a kernel that writes past a capacity, before
its output or into an entry it should leave alone goes unseen there. A Guard is one allocation
of `margin + shift + nbytes + margin` bytes filled with SENTINEL; the kernel gets the address
`base + margin + shift` (shift = 0 keeps the 256-byte alignment of the allocation, a non-zero one
misaligns the payload on purpose) and the test reads the whole allocation back:

    g = Guard(arena, n, R.INST_STATE)          # an output the kernel writes
    engine.some_call_dev(..., g.ptr, ...)
    engine.synchronize()
    g.assert_margins()                         # nothing before or after the payload changed
    g.assert_untouched(~touched)               # these payload elements still hold the sentinel
    got = g.payload()

Built on minpaxos_amd.devbuf.Arena: the allocation is freed with the arena.
"""
import ctypes as C

import numpy as np

from minpaxos_amd.devbuf import D2H, H2D

SENTINEL = 0xA5
MARGIN = 256


class Guard:
    def __init__(self, arena, shape, dtype, shift=0, margin=MARGIN, name=None):
        assert margin >= 256 and margin % 256 == 0 and 0 <= shift < 256
        self.ar, self.eng = arena, arena.eng
        self.shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
        self.dtype = np.dtype(dtype)
        self.count = int(np.prod(self.shape))
        self.nbytes = self.count * self.dtype.itemsize
        self.margin, self.shift, self.name = margin, shift, name or str(self.dtype)
        self.total = margin + shift + self.nbytes + margin
        self.base = arena.empty(self.total, np.uint8).ptr
        self.ptr = self.base + margin + shift
        self.fill()
        self.eng.stream_synchronize(None)

    def at(self, index):
        """device pointer of payload element `index`"""
        return self.ptr + int(index) * self.dtype.itemsize

    def fill(self, stream=None):
        """the whole allocation back to the sentinel (asynchronous on `stream`)"""
        self.eng.memset(self.base, SENTINEL, self.total, stream)

    def put(self, a, stream=None):
        """host array -> payload (an in/out buffer); returns self"""
        a = np.ascontiguousarray(a, self.dtype)
        assert a.nbytes == self.nbytes, (self.name, a.nbytes, self.nbytes)
        if a.nbytes:
            self.eng.memcpy(self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D, stream)
            self.eng.stream_synchronize(stream)
        return self

    def raw(self, stream=None):
        """the whole allocation, margins included, as bytes"""
        out = np.empty(self.total, np.uint8)
        self.eng.memcpy(out.ctypes.data_as(C.c_void_p), self.base, self.total, D2H, stream)
        self.eng.stream_synchronize(stream)
        return out

    def payload(self, stream=None):
        lo = self.margin + self.shift
        return self.raw(stream)[lo:lo + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def assert_margins(self, stream=None):
        """fails, naming the first touched offset (relative to the payload), if any byte before
        or after the payload changed"""
        raw = self.raw(stream)
        lo = self.margin + self.shift
        outside = np.ones(self.total, bool)
        outside[lo:lo + self.nbytes] = False
        bad = np.flatnonzero(outside & (raw != SENTINEL))
        if len(bad):
            o = int(bad[0])
            raise AssertionError(
                f"{self.name}: guard byte at payload offset {o - lo} (payload is {self.nbytes} "
                f"bytes, shift {self.shift}) was overwritten with {int(raw[o]):#04x}; "
                f"{len(bad)} guard bytes changed in all")
        return raw[lo:lo + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def assert_untouched(self, mask_or_ranges, stream=None):
        """the named payload elements still hold the sentinel: a boolean mask over the (flattened)
        payload elements, or a list of (lo, hi) element ranges"""
        if isinstance(mask_or_ranges, np.ndarray) and mask_or_ranges.dtype == bool:
            mask = mask_or_ranges.reshape(-1)
            assert len(mask) == self.count, (self.name, len(mask), self.count)
        else:
            mask = np.zeros(self.count, bool)
            for lo, hi in mask_or_ranges:
                assert 0 <= lo <= hi <= self.count, (self.name, lo, hi, self.count)
                mask[lo:hi] = True
        if not self.count:
            return
        by = self.payload(stream).reshape(-1).view(np.uint8).reshape(self.count, -1)
        bad = np.flatnonzero(mask & (by != SENTINEL).any(axis=1))
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{self.name}: element {i} should have been left alone but holds "
                                 f"{by[i].tobytes().hex()}; {len(bad)} such elements in all")


def sentinel_array(shape, dtype):
    """what an untouched payload reads back as"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, SENTINEL, np.uint8).view(dtype).reshape(shape)
