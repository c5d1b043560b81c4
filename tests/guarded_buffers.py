"""Guarded device regions and poison fills for tests that call a C entry point of libchebgcn.so directly (plain helpers, no
fixtures; tests/test_gpu_analysis_buffers.py, tests/test_gpu_staging_kernels.py and their host companions use them).

``Guarded`` generalises the float-only ``Guarded`` classes of test_gpu_head_kernels.py, test_gpu_fused_layer_arms.py and
test_gpu_attribution_kernels.py (which stay as they are): a region of ANY dtype and byte size inside one larger allocation,
between two guard bands of at least ``GUARD_BYTES`` bytes that hold ``GUARD_BYTE``, starting at the WEAKEST alignment the
entry's argument check admits (``align`` = 4, 8 or 16: the address is a multiple of ``align`` and not of ``2 * align``), so a
kernel that assumes more than the header promises faults its own check, and one that stores a few elements past its output or
its declared workspace changes a band instead of allocator slack.  The interior is pre-filled with a poison.

Poison pairs.  Every case runs twice, into fresh regions: fill A is all bytes 0xFF (NaN as float32 / float64, -1 as an
integer), fill B all bytes 0x5A (a finite, large, wrong number: 1.5e16 as float32, 4e125 as float64; 1515870810 as int32).  A
kernel that reads memory nobody wrote gives two different answers (or NaN); one that leaves a part of an output unwritten
leaves the two fills there.  Zero is never a fill: a forgotten memset would go unnoticed.
"""
import ctypes

import numpy as np

GUARD_BYTES = 4096
GUARD_BYTE = 0xC3
FILL_A = 0xFF
FILL_B = 0x5A
FILLS = (('A', FILL_A), ('B', FILL_B))

_NP = {'float32': np.float32, 'float64': np.float64, 'int32': np.int32, 'int64': np.int64, 'uint8': np.uint8}


def fill_value(fill, dtype):
    """The scalar every element of ``dtype`` (a NumPy dtype or its name) holds in a region whose bytes are all ``fill``."""
    dt = np.dtype(_NP.get(dtype, dtype))
    return np.full(dt.itemsize, fill, np.uint8).view(dt)[0]


def filled(fill, dtype, shape):
    """A host array of ``shape`` whose bytes are all ``fill``."""
    dt = np.dtype(_NP.get(dtype, dtype))
    return np.full(int(np.prod(shape, dtype=np.int64)) * dt.itemsize, fill, np.uint8).view(dt).reshape(shape)


def bits(a):
    """The bytes of a host array as an unsigned integer array of the same shape (NaN compares equal to the same NaN)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def layout(base_address, nbytes, align):
    """``(offset of the region, bytes of the whole allocation)`` for an allocation that starts at ``base_address``: the region
    starts at least GUARD_BYTES in, at an address that is an odd multiple of ``align``; at least GUARD_BYTES follow it."""
    assert align in (1, 4, 8, 16) and nbytes >= 0
    start = base_address + GUARD_BYTES
    start += (-start) % (2 * align) + align if align > 1 else 1
    off = start - base_address
    return off, off + nbytes + GUARD_BYTES + 2 * align


class Guarded:
    """A device region of ``shape`` x ``dtype`` (a NumPy dtype name) between two guard bands, pre-filled with the byte
    ``fill``.  ``t``: the region as a torch tensor of that shape (``init`` -- a host array -- is copied into it, ``base``
    -- a scalar -- fills it, for buffers a call adds into or updates in place); ``ptr``: its address for ctypes; ``nbytes``."""

    def __init__(self, shape, dtype, fill, dev, align=16, init=None, base=None):
        import torch
        self.np_dtype = np.dtype(_NP[dtype])
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.np_dtype.itemsize
        assert align >= min(self.np_dtype.itemsize, 16) and align % self.np_dtype.itemsize == 0, (dtype, align)
        # the allocator's own alignment is not assumed: allocate for the worst case, then lay the region out from the address
        self.whole = torch.full((GUARD_BYTES + self.nbytes + GUARD_BYTES + 4 * align + 64,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.off, used = layout(self.whole.data_ptr(), self.nbytes, align)
        assert used <= self.whole.numel()
        self.raw = self.whole[self.off:self.off + self.nbytes]
        self.raw.fill_(fill)
        self.t = self.raw.view(getattr(torch, dtype)).view(self.shape) if self.nbytes else None
        self.address = self.whole.data_ptr() + self.off
        assert self.address % align == 0 and (align == 1 or self.address % (2 * align) != 0)
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init, self.np_dtype)).view(self.shape))
        elif base is not None:
            self.t.fill_(base)
        self.ptr = ctypes.c_void_p(self.address)

    def bands_intact(self):
        lo, hi = self.whole[:self.off], self.whole[self.off + self.nbytes:]
        return bool((lo == GUARD_BYTE).all()) and bool((hi == GUARD_BYTE).all())

    def check(self, what):
        """Both guard bands are byte-identical to the pattern."""
        import torch
        for side, band, first in (('in front of', self.whole[:self.off], 0),
                                  ('behind', self.whole[self.off + self.nbytes:], self.off + self.nbytes)):
            bad = torch.nonzero(band != GUARD_BYTE).flatten()
            assert bad.numel() == 0, '%s: guard changed -- %d bytes of the band %s the region, the nearest %d bytes %s it' % (
                what, bad.numel(), side, (self.off - int(bad[-1])) if first == 0 else int(bad[0]) + 1, side)

    def host(self):
        """The region's content as a host array of its dtype and shape."""
        return self.raw.cpu().numpy().view(self.np_dtype).reshape(self.shape).copy()
