"""Guard-banded placement of kernel arguments at chosen alignments and leading dimensions.

The entry points of include/mri_inr.h pick 16-byte or 4-byte accesses from the alignment of a pointer, from a
leading dimension and from where a row range ends.  Freshly allocated, contiguous torch tensors only ever show
them one side of those predicates, and a comparison of an output tensor cannot see a store that lands one
float past its end.  `place` puts a tensor at a chosen offset inside a buffer of sentinels, so that a test
picks the branch and then proves that nothing outside the logical elements was written.
"""
import ctypes as C

import torch

# a quiet NaN with a payload: no kernel computes it, and a float that was overwritten with ANY value differs
SENTINEL = 0x7FC0BEEF
OFFSETS = (1, 2, 3)  # floats: the three misaligned positions inside a 16-byte line


def place(values, offset_floats, ld=None, guard=64):
    """Copy `values` (1-D or 2-D, float32) `guard + offset_floats` floats into a flat CUDA buffer of sentinels,
    rows `ld` floats apart (default: packed).  Returns (view, check): `view` aliases the buffer with
    view.data_ptr() % 16 == 4 * (offset_floats % 4); check(unchanged=False, what="") asserts, bit for bit, that
    every float outside the logical elements (both guards and the padding columns of a wide `ld`) still holds
    the sentinel and, with unchanged=True, that the logical elements hold what was placed (an input)."""
    v = torch.as_tensor(values, dtype=torch.float32)
    assert v.dim() in (1, 2) and guard % 4 == 0 and offset_floats >= 0
    rows, width = (1, v.numel()) if v.dim() == 1 else v.shape
    ld_ = width if ld is None else int(ld)
    assert ld_ >= width
    span = (rows - 1) * ld_ + width if rows else 0
    start = guard + offset_floats
    total = (start + span + guard + 3) // 4 * 4
    buf = torch.empty(total, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    bits = buf.view(torch.int32)
    bits.fill_(SENTINEL)
    size, stride = ((width,), (1,)) if v.dim() == 1 else ((rows, width), (ld_, 1))
    view = buf.as_strided(size, stride, start)
    view.copy_(v)
    assert view.data_ptr() % 16 == 4 * (offset_floats % 4)
    logical = torch.zeros(total, dtype=torch.bool, device="cuda")
    logical.as_strided(size, stride, start).fill_(True)
    placed = bits.as_strided(size, stride, start).clone()

    def check(unchanged=False, what=""):
        torch.cuda.synchronize()
        stray = ((bits != SENTINEL) & ~logical).nonzero().flatten()
        assert stray.numel() == 0, (f"{what}: {stray.numel()} floats outside the tensor were written, the first "
                                    f"{int(stray[0]) - start} floats from its start (ld {ld_}, width {width})")
        if unchanged:
            assert torch.equal(bits.as_strided(size, stride, start), placed), f"{what}: an input was modified"

    return view, check


def place_workspace(n_bytes, fill, guard_bytes=None):
    """A kernel workspace of exactly `n_bytes` (rounded up to the next multiple of 16 for the buffer's own
    bookkeeping; the call is still told n_bytes) whose start is 16-byte aligned, inside ONE CUDA buffer between two
    guards of SENTINEL words.  `fill` is the 32-bit pattern the workspace itself holds before the call.  Each guard
    is at least 1 MiB and at least a quarter of n_bytes (or `guard_bytes`): a slab count that is off by a few
    workgroups writes into the guard, not outside the allocation.  Returns (workspace, check): `workspace` is the
    int32 view to take the pointer of (a NULL pointer when n_bytes is 0); check(what) asserts, bit for bit, that
    both guards are intact and says how many bytes past the end (or before the start) the first stray write lies."""
    n_bytes = int(n_bytes)
    assert n_bytes >= 0 and 0 <= fill < 1 << 32
    body = (n_bytes + 15) // 16 * 16
    guard = max(1 << 20, (n_bytes + 3) // 4) if guard_bytes is None else int(guard_bytes)
    guard = (guard + 15) // 16 * 16
    g, b = guard // 4, body // 4
    buf = torch.empty(2 * g + b, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(SENTINEL)
    ws = buf[g:g + b]
    ws.fill_(fill - (1 << 32) if fill >= 1 << 31 else fill)
    assert b == 0 or ws.data_ptr() % 16 == 0

    def check(what=""):
        torch.cuda.synchronize()
        after = (buf[g + b:] != SENTINEL).nonzero().flatten()
        assert after.numel() == 0, (f"{what}: {after.numel()} words behind a workspace of {n_bytes} bytes were written, "
                                    f"the first {body + 4 * int(after[0]) - n_bytes} bytes past its end")
        before = (buf[:g] != SENTINEL).nonzero().flatten()
        assert before.numel() == 0, (f"{what}: {before.numel()} words in front of the workspace were written, the "
                                     f"nearest {4 * (g - int(before[-1]))} bytes before its start")

    return ws, check


def variants(widths, lds=True):
    """Layouts of a call's arguments: {name: width of a row, or None for an argument without a leading
    dimension} -> [(tag, {name: (offset, ld)})]: all aligned and packed (the FAST path, under guards too), each
    argument alone at offsets 1, 2, 3 and at ld = width + 1, + 3, + 4, and all arguments shifted together."""
    base = {name: (0, None) for name in widths}
    out = [("aligned", base)]
    for name, width in widths.items():
        for off in OFFSETS:
            out.append((f"{name} + {off}", {**base, name: (off, None)}))
        if width is not None and lds:
            for ld in (width + 1, width + 3, width + 4):
                out.append((f"{name} ld {ld}", {**base, name: (0, ld)}))
    out.append(("all shifted", {name: (1 + i % 3, None if width is None or not lds else width + 1 + 2 * (i % 2))
                                for i, (name, width) in enumerate(widths.items())}))
    return out


class Placer:
    """The arguments of one call under one layout: inp() / out() place them, verify() runs every check."""

    def __init__(self, layout, tag=""):
        self.layout, self.tag, self.checks = layout, tag, []

    def _put(self, name, values, is_input, ld=None):
        off, own_ld = self.layout.get(name, (0, None))
        ld = own_ld if ld is None else ld
        view, check = place(values, off, ld if torch.as_tensor(values).dim() == 2 else None)
        self.checks.append((name, check, is_input))
        return view

    def inp(self, name, values, ld=None):
        return self._put(name, values, True, ld)

    def out(self, name, shape, fill=float("nan"), ld=None):
        """An output; NaN-filled unless the call accumulates into it, so that an element nobody stored fails
        every comparison.  `ld`: a leading dimension the call shares with another argument."""
        return self._put(name, torch.full(shape, fill, dtype=torch.float32), False, ld)

    def verify(self):
        for name, check, is_input in self.checks:
            check(unchanged=is_input, what=f"{self.tag}: {name}")


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None
