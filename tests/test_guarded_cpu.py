"""The guarded-buffer harness (tests/guarded.py) proves itself without a GPU: the CPU oracle stands in for the kernels on
HostArena views -- a correct call passes, and every kind of fault the GPU tests are meant to catch is planted once and caught."""

import ctypes as C

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.signals import noise

M, N_SAMPLES = 24, 300


def qnan(a) -> np.ndarray:
    return np.isnan(np.asarray(a).view(np.asarray(a).real.dtype))


def analysis_call(combo, res_x=0, res_out=0, modulus=16):
    """The oracle's analysis on guarded host views: (arena, x view, out view, expected matrix)."""
    td, fd, fdx = O.combo_types(combo)
    x = noise(N_SAMPLES, seed=3, dtype=td)
    want = O.best(M, "hann", 1.0, combo).sdft(x)
    arena = G.HostArena(G.room(((N_SAMPLES,), td), ((N_SAMPLES, M), fdx)))
    xv = G.put(arena.carve((N_SAMPLES,), td, res_x, modulus, name="samples"), x)
    out = arena.carve((N_SAMPLES, M), fdx, res_out, modulus, name="dfts")
    return arena, xv, out, want


def test_sentinels_are_quiet_nans_at_every_type():
    for word in (G.GUARD_WORD, G.UNWRITTEN_WORD):
        raw = np.resize(np.array([word], dtype="<u4").view(np.uint8), 64)
        f32, f64 = raw.view(np.float32), raw.view(np.float64)
        assert np.all(np.isnan(f32)) and np.all(np.isnan(f64))
        assert np.all(raw.view(np.uint32) & 0x00400000) and np.all(raw.view(np.uint64) & (1 << 51))     # quiet bits
        assert np.all(np.isnan(raw.view(np.complex64))) and np.all(np.isnan(raw.view(np.complex128)))
    assert G.GUARD_WORD != G.UNWRITTEN_WORD


@pytest.mark.parametrize("dtype,residues", [(np.float32, (0, 4, 8, 12)), (np.float64, (0, 8)), (np.complex64, (0, 8)), (np.complex128, (0,))])
def test_carve_delivers_every_residue(dtype, residues):
    arena = G.HostArena(4 << 20)
    for r in residues:
        v = arena.carve((5, 7), dtype, r)
        assert v.ctypes.data % 16 == r and v.flags.c_contiguous and v.dtype == dtype and v.shape == (5, 7)
        assert G.view_unwritten(v) == v.size and np.all(qnan(v))
    for r in (16, 80):
        v = arena.carve((33,), dtype, r, modulus=128)
        assert v.ctypes.data % 128 == r
    with pytest.raises(AssertionError):
        arena.carve((4,), dtype, np.dtype(dtype).itemsize // 2)           # not an address of an element
    # guards: at least 64 KiB, and two rows where rows are longer
    starts = sorted((w.start, w.end, w.guard) for w in arena.views)
    assert starts[0][0] >= G.MIN_GUARD
    for (s0, e0, g0), (s1, e1, g1) in zip(starts, starts[1:]):
        assert s1 - e0 >= max(g0, g1) >= G.MIN_GUARD
    assert arena.nbytes - starts[-1][1] >= starts[-1][2]
    wide = G.HostArena(G.room(((3, 40000), np.complex128)))
    wide.carve((3, 40000), np.complex128, 0)
    assert wide.views[0].guard == 2 * 40000 * 16 and wide.views[0].start >= wide.views[0].guard
    arena.check(); wide.check()
    with pytest.raises(ValueError):
        G.HostArena(100 << 10).carve((1 << 14,), np.float64, 0)            # no room for the trailing guard


@pytest.mark.parametrize("combo", O.COMBOS)
def test_a_correct_call_passes(combo):
    td, fd, fdx = O.combo_types(combo)
    res = [r for r in (0, 4, 8, 12) if r % np.dtype(td).itemsize == 0]
    for res_x in res:
        for res_out in ((0, 8) if fd == np.float32 else (0,)):
            arena, xv, out, want = analysis_call(combo, res_x, res_out)
            assert G.view_unwritten(out) == out.size
            O.best(M, "hann", 1.0, combo).sdft(xv, out=out)
            arena.check()
            assert G.view_unwritten(out) == 0 and G.view_unwritten(xv) == 0
            assert np.array_equal(out, want)
    arena, xv, out, want = analysis_call(combo, 16, 80, modulus=128)
    O.best(M, "hann", 1.0, combo).sdft(xv, out=out)
    arena.check()
    assert np.array_equal(out, want)


@pytest.mark.parametrize("where,elements", [("after", 1), ("before", 1), ("after", 3)])
def test_a_store_outside_the_view_is_caught_and_located(where, elements):
    """A kernel that stores `elements` bins past the last row, or before the first."""
    arena, xv, out, want = analysis_call("f32f32", 4, 8)
    ref = O.best(M, "hann", 1.0, "f32f32")
    ref.sdft(xv, out=out)
    item = out.dtype.itemsize
    addr = out.ctypes.data + (out.size * item if where == "after" else -elements * item)
    C.memmove(addr, np.zeros(elements, dtype=out.dtype).ctypes.data, elements * item)        # the planted store
    with pytest.raises(G.GuardError) as e:
        arena.check()
    text = str(e.value)
    if where == "after":
        assert f"first byte 1 bytes past the last byte of 'dfts'" in text and f"last byte {elements * item} bytes past the last byte of 'dfts'" in text
    else:
        assert f"first byte {elements * item} bytes before the start of 'dfts'" in text and "last byte 1 bytes before the start of 'dfts'" in text
    assert np.array_equal(out, want)                                     # the view itself was right: only the guard tells


def test_a_single_dirtied_byte_is_caught():
    arena, xv, out, want = analysis_call("f64f64")
    arena.bytes[arena.views[0].start - 1] ^= 1                             # one bit of the byte before the samples
    with pytest.raises(G.GuardError, match="1 bytes before the start of 'samples'"):
        arena.check()


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("shift", [-1, 1])
def test_a_read_outside_the_input_reaches_the_result(combo, shift):
    """A kernel that reads x[-1] (shift -1) or x[n] (shift +1): the guard's NaN enters the recurrence, and the matrix is no
    longer the oracle's."""
    td, fd, fdx = O.combo_types(combo)
    arena, xv, out, want = analysis_call(combo, np.dtype(td).itemsize % 16, 0)
    shifted = np.frombuffer((C.c_char * (xv.size * xv.itemsize)).from_address(xv.ctypes.data + shift * xv.itemsize), dtype=td)
    O.best(M, "hann", 1.0, combo).sdft(shifted, out=out)                   # the planted read
    arena.check()                                                          # nothing was stored outside ...
    assert G.view_unwritten(out) == 0
    assert not np.array_equal(out, want) and qnan(out).any()               # ... but the result shows it


def test_a_read_outside_the_matrix_reaches_the_samples():
    """The synthesis reading one bin past the last row."""
    td, fd, fdx = O.combo_types("f32f64")
    x = noise(N_SAMPLES, seed=5, dtype=td)
    d = O.best(M, "hann", 0.5, "f32f64").sdft(x)
    want = O.best(M, "hann", 0.5, "f32f64").isdft(d)
    arena = G.HostArena(G.room(((N_SAMPLES, M), fdx), ((N_SAMPLES,), td)))
    dv = G.put(arena.carve((N_SAMPLES, M), fdx, 0, name="dfts"), d)
    y = arena.carve((N_SAMPLES,), td, 12, name="samples")
    O.best(M, "hann", 0.5, "f32f64").isdft(dv, out=y)
    arena.check()
    assert np.array_equal(y, want)
    off = np.frombuffer((C.c_char * dv.nbytes).from_address(dv.ctypes.data + dv.itemsize), dtype=fdx).reshape(N_SAMPLES, M)
    O.best(M, "hann", 0.5, "f32f64").isdft(off, out=y)
    assert np.isnan(y[-1]) and not np.array_equal(y, want)


def test_a_skipped_element_is_counted():
    """A kernel that leaves holes: the last bin of every 7th row and one whole row."""
    arena, xv, out, want = analysis_call("f64f32", 8, 8)
    out[...] = want
    assert G.view_unwritten(out) == 0
    hole = np.resize(np.array([G.UNWRITTEN_WORD], dtype=np.uint32), 2).view(np.complex64)[0]
    out[::7, -1] = hole
    out[5, :] = hole
    rows7 = len(range(0, N_SAMPLES, 7))
    assert G.view_unwritten(out) == rows7 + M - (1 if 5 % 7 == 0 else 0)
    arena.check()
    # half an element written is an element written: only a whole untouched element counts
    out[9, 0] = complex(1.0, float(hole.imag))
    assert G.view_unwritten(out) == rows7 + M
