"""Guarded, deliberately misaligned buffers for the tests.  TEST HELPER (plain module, imported like exact_sdft).

An arena is ONE flat byte allocation -- a torch uint8 CUDA tensor (DeviceArena) or a page-aligned numpy array (HostArena) --
filled completely with a sentinel.  carve() cuts contiguous views out of it at a chosen residue of the address, with a
guard of at least max(64 KiB, 2 rows) on either side of every view.  Inputs are copied into their views (put), outputs
start as the "not yet written" sentinel.  After the call under test

    arena.check()          every byte outside the views still holds the guard pattern (byte for byte; the report names the
                           first and last dirtied byte relative to the nearest view)
    view_unwritten(view)   elements of a view that still hold the "not yet written" pattern (holes in an output)

and an out-of-range LOAD that reaches a result shows as a NaN or a broken bit-identity, because everything outside the
inputs is NaN.  A masked over-read that is discarded stays legal, and cannot fault: the guard is part of the same allocation.

The sentinels.  Both patterns repeat one 32-bit word, so they read the same at every 4-byte aligned address:
    guard      0x7FFA5A5A   float32: exponent 0xFF, quiet bit set, payload 0x3A5A5A -> quiet NaN
                            float64 0x7FFA5A5A7FFA5A5A: exponent 0x7FF, bit 51 set          -> quiet NaN
    unwritten  0x7FFC3C3C   likewise (0x7FFC3C3C7FFC3C3C)
complex64 / complex128 are pairs of those.  No arithmetic produces either payload, so an element that equals one was not
written by the code under test.
"""

from __future__ import annotations

import math

import numpy as np

GUARD_WORD = 0x7FFA5A5A
UNWRITTEN_WORD = 0x7FFC3C3C
MIN_GUARD = 64 << 10
PAGE = 4096


def _word_bytes(word: int) -> np.ndarray:
    return np.array([word], dtype="<u4").view(np.uint8)


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _np_dtype(dtype) -> np.dtype:
    if isinstance(dtype, np.dtype) or not type(dtype).__module__.startswith("torch"):
        return np.dtype(dtype)
    return np.dtype(str(dtype).split(".")[-1])


class _View:
    def __init__(self, name, start, nbytes, guard):
        self.name, self.start, self.nbytes, self.guard = name, start, nbytes, guard

    @property
    def end(self):
        return self.start + self.nbytes


class GuardError(AssertionError):
    pass


class _Arena:
    """Shared bookkeeping; the subclasses supply the memory (_alloc), its address, filling, reading and slicing."""

    def __init__(self, nbytes: int):
        self.nbytes = (int(nbytes) + 3) // 4 * 4
        self._alloc(self.nbytes)
        self._fill(0, self.nbytes, GUARD_WORD)
        self.views: list[_View] = []
        self._cursor = 0

    # -- carving --------------------------------------------------------------------------------------------------------
    def carve(self, shape, dtype, byte_offset_mod: int = 0, modulus: int = 16, guard: int | None = None, name: str | None = None):
        """A contiguous view of `shape` / `dtype` with data_ptr() % modulus == byte_offset_mod, `guard` bytes (default and
        minimum: max(64 KiB, 2 rows)) of guard pattern on both sides, its own bytes set to the "not yet written" pattern."""
        dt = _np_dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        align = min(dt.itemsize, 16)
        assert modulus % align == 0 and 0 <= byte_offset_mod < modulus and byte_offset_mod % align == 0, \
            f"residue {byte_offset_mod} mod {modulus} is not an address of a {dt} element"
        row = (shape[-1] if len(shape) >= 2 else 1) * dt.itemsize
        least = max(MIN_GUARD, 2 * row)
        guard = least if guard is None else max(int(guard), least)
        nbytes = math.prod(shape) * dt.itemsize
        start = self._cursor + guard
        start += (byte_offset_mod - (self.base + start)) % modulus
        end = start + nbytes
        if end + guard > self.nbytes:
            raise ValueError(f"arena of {self.nbytes} bytes is too small: view needs bytes up to {end + guard}")
        v = _View(name or f"view{len(self.views)}", start, nbytes, guard)
        self.views.append(v)
        self._cursor = end + guard
        self._fill(start, nbytes, UNWRITTEN_WORD)
        out = self._typed(start, nbytes, dt, shape)
        assert nbytes == 0 or (ptr_of(out) % modulus == byte_offset_mod and ptr_of(out) == self.base + start)   # (torch: an empty view has no address)
        return out

    @staticmethod
    def room(*views, guard: int = MIN_GUARD) -> int:
        """Bytes an arena needs for views given as (shape, dtype) pairs, default guards, any residue up to modulus 256."""
        total = 0
        for shape, dtype in views:
            dt = _np_dtype(dtype)
            shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
            row = (shape[-1] if len(shape) >= 2 else 1) * dt.itemsize
            total += math.prod(shape) * dt.itemsize + 2 * max(guard, MIN_GUARD, 2 * row) + 512
        return total + 512

    # -- checking -------------------------------------------------------------------------------------------------------
    def _gaps(self):
        at = 0
        for v in sorted(self.views, key=lambda v: v.start):
            if v.start > at:
                yield at, v.start
            at = v.end
        if at < self.nbytes:
            yield at, self.nbytes

    def _nearest(self, off: int) -> str:
        best = None
        for v in self.views:
            d = off - v.start if off < v.start else off - (v.end - 1) if off >= v.end else 0
            if best is None or abs(d) < abs(best[0]):
                best = (d, v)
        if best is None:
            return f"arena byte {off}"
        d, v = best
        return f"{-d} bytes before the start of '{v.name}'" if d < 0 else f"{d} bytes past the last byte of '{v.name}'"

    def dirty(self):
        """(first, last) arena offsets of guard bytes that no longer hold the pattern, or None."""
        first = last = None
        for a, b in self._gaps():
            got = self._read(a, b - a)
            want = np.resize(np.roll(_word_bytes(GUARD_WORD), -(a % 4)), b - a)
            bad = np.flatnonzero(got != want)
            if bad.size:
                first = a + int(bad[0]) if first is None else first
                last = a + int(bad[-1])
        return None if first is None else (first, last)

    def check(self):
        """Asserts that every guard byte still holds the guard pattern."""
        d = self.dirty()
        if d is not None:
            raise GuardError(f"guard dirtied: first byte {self._nearest(d[0])}, last byte {self._nearest(d[1])} "
                             f"(arena offsets {d[0]} .. {d[1]})")


class HostArena(_Arena):
    """One page-aligned numpy allocation (so that offsets are exact residues of the address)."""

    def _alloc(self, nbytes):
        self._raw = np.empty(nbytes + PAGE, dtype=np.uint8)
        skip = (-self._raw.ctypes.data) % PAGE
        self.bytes = self._raw[skip:skip + nbytes]
        self.base = self.bytes.ctypes.data
        assert self.base % PAGE == 0

    def _fill(self, start, nbytes, word):
        self.bytes[start:start + nbytes] = np.resize(np.roll(_word_bytes(word), -(start % 4)), nbytes)

    def _read(self, start, nbytes):
        return self.bytes[start:start + nbytes]

    def _typed(self, start, nbytes, dt, shape):
        return self.bytes[start:start + nbytes].view(dt).reshape(shape)


class DeviceArena(_Arena):
    """One torch uint8 CUDA tensor."""

    def _alloc(self, nbytes):
        import torch
        self.bytes = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.base = self.bytes.data_ptr()
        assert self.base % 256 == 0

    def _fill(self, start, nbytes, word):
        import torch
        assert start % 4 == 0 and nbytes % 4 == 0
        self.bytes[start:start + nbytes].view(torch.int32).fill_(int(np.array([word], dtype=np.uint32).view(np.int32)[0]))

    def _read(self, start, nbytes):
        return self.bytes[start:start + nbytes].cpu().numpy()

    def _typed(self, start, nbytes, dt, shape):
        import torch
        return self.bytes[start:start + nbytes].view(getattr(torch, dt.name)).view(shape)


room = _Arena.room


def ptr_of(view) -> int:
    return int(view.data_ptr()) if _is_tensor(view) else int(view.ctypes.data)


def put(view, values):
    """Copies an input into its view (bits and all)."""
    if _is_tensor(view):
        import torch
        view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=_np_dtype(view.dtype)).reshape(tuple(view.shape))))
    else:
        view[...] = np.asarray(values, dtype=view.dtype).reshape(view.shape)
    return view


def to_numpy(view) -> np.ndarray:
    return view.cpu().numpy() if _is_tensor(view) else np.array(view, copy=True)


def view_unwritten(view) -> int:
    """Elements of the view that still hold the "not yet written" pattern."""
    a = np.ascontiguousarray(to_numpy(view))
    if a.size == 0:
        return 0
    words = a.reshape(-1).view(np.uint32).reshape(a.size, -1)
    return int(np.all(words == np.uint32(UNWRITTEN_WORD), axis=1).sum())
