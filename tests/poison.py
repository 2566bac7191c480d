"""Poisoned allocations for the test-suite: make memory that nobody wrote visible.

The package allocates every workspace, split-K slab, partial sum and output with `torch.empty` / `torch.empty_like`.  On the
GPU the caching allocator hands back recycled memory; in a test that memory is often fresh or holds finite leftovers, so a
kernel that skips a ragged tile, the last slab or the last chunk -- or multiplies a pad column it never wrote by a zero
weight (0 * NaN = NaN) -- can pass by luck.  Under `poisoned_allocations()` every such buffer starts out as NaN instead.

TEST INFRASTRUCTURE ONLY: the product never imports this module.
"""
import contextlib

import torch

# int16 tensors are the bf16 hi / lo operand planes: 0x7FC0 is the bf16 quiet NaN
BF16_NAN_BITS = 0x7FC0
# every other integer dtype: one fixed, non-zero byte pattern
_INT_POISON = {torch.uint8: 0x5A, torch.int8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}


def poison_(t):
    """Fill t in place with the poison value of its dtype (meta and zero-size tensors are left alone); returns t."""
    if t.device.type == "meta" or t.numel() == 0:
        return t
    with torch.no_grad():
        if t.dtype.is_floating_point or t.dtype.is_complex:
            t.fill_(float("nan"))
        elif t.dtype == torch.int16:
            t.fill_(BF16_NAN_BITS)
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(_INT_POISON.get(t.dtype, 0x5A))
    return t


@contextlib.contextmanager
def poisoned_allocations():
    """While active, torch.empty, torch.empty_like and Tensor.new_empty return tensors already filled with poison."""
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def p_empty(*a, **k):
        return poison_(empty(*a, **k))

    def p_empty_like(*a, **k):
        return poison_(empty_like(*a, **k))

    def p_new_empty(self, *a, **k):
        return poison_(new_empty(self, *a, **k))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = p_empty, p_empty_like, p_new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty


def nan_empty(be, *shape, dtype=torch.float32):
    """A kernel-level test's output / workspace / pad-column buffer on backend `be` (tests/conftest.py: Backend), poisoned.
    Use it for every buffer a kernel's contract says it overwrites; buffers whose pad columns the product guarantees to be
    zero (new_feat(zero=True) when C % 4) stay torch.zeros."""
    return poison_(torch.empty(*shape, device=be.device, dtype=dtype))


GUARD = 4096          # floats on either side of every output


class Guarded:
    """n output tensors of one shape carved out of a single poisoned buffer, GUARD floats apart."""

    def __init__(self, dev, shape, n):
        self.numel = 1
        for s in shape:
            self.numel *= s
        self.stride = self.numel + GUARD
        self.buf = torch.empty(GUARD + n * self.stride, device=dev, dtype=torch.float32)
        self.outs = [self.buf[GUARD + i * self.stride: GUARD + i * self.stride + self.numel].view(shape) for i in range(n)]
        self.mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=dev)
        for i in range(n):
            self.mask[GUARD + i * self.stride: GUARD + i * self.stride + self.numel] = False

    def poison(self):
        poison_(self.buf)

    def guards_intact(self):
        return bool(torch.isnan(self.buf[self.mask]).all())
