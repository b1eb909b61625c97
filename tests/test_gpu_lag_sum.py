"""Lag-product analysis (sdft_hip_sdft_lag_sum_n, SDFT.lag_sum) on a real MI355X against the oracle's rows.

The term of sample t is A conj(B), A the oracle's row of sample t and B its row of sample t - 1 (the zero row before a fresh plan's
first sample), written on real arrays in the FD dtype with one rounding per operation:

    re = ar * br + ai * bi          im = ai * br - ar * bi

At every = 1, first = 0 a row IS its term, so on the bit-identical routes (FD float, FD double with carry = 1, calls of one time
chunk) the comparison is bit for bit, from the second term on; the first term of a fresh plan is zero as a number.  On other grids
the bar is, per component, with L the window's length, u = 2^-24 (float) or 2^-53 (double), gamma_n = n u / (1 - n u), T = sum
|term| over the window and S the terms' exact sum: |sum - S| <= gamma_(L-1) T (promise 3 of the header).  S and T are formed in
float64 (FD float) or in an extended long double (FD double), whose own error, at most L uw T with uw = 2^-53 / 2^-64, is added to
the bar (1/2048 of it or less).  For FD double with default carries L * 2.1e-11 * max |X|^2 over the call's rows and band comes on
top (promise 4).

Inputs are sine_sweep(n) + 0.25 noise(n), the signal of tests/test_gpu_power.py."""

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import every_next_first, lag_frequency, power_sum_rows
from test_gpu_power import BAR, WINDOWS, exact_combo, make, signal, to_dev
from test_gpu_power_sum import GRIDS, wide, windows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [("f32f32", {}), ("f32f64", {"carry": 1})]           # a bit-identical route of either FD type
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the FD double reference needs an extended long double"


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def oracle_rows(ref, x, block=2048):
    """(len(x), dftsize) rows of the oracle, fed in blocks"""
    return np.concatenate([ref.sdft(x[t:t + block]) for t in range(0, x.size, block)]) if x.size else np.empty((0, ref.dftsize), dtype=ref.fdx)


@functools.lru_cache(maxsize=6)
def rows_of(combo, window, m, n, seed=None):
    """(samples, rows) of one shape from a fresh oracle; computed once, shared, never written"""
    td = O.combo_types(combo)[0]
    x = signal(n, td, m if seed is None else seed)
    X = oracle_rows(O.best(m, window, 1.0, combo), x)
    x.setflags(write=False)
    X.setflags(write=False)
    return x, X


def terms_of(X, prev=None):
    """(re, im) of A conj(B) for the rows X and the rows before them (prev: the row before X[0], None: the zero row)"""
    B = np.concatenate([np.zeros((1, X.shape[1]), dtype=X.dtype) if prev is None else np.asarray(prev, dtype=X.dtype)[None], X[:-1]])
    ar, ai = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    br, bi = np.ascontiguousarray(B.real), np.ascontiguousarray(B.imag)
    re = ar * br + ai * bi
    im = ai * br - ar * bi
    assert re.dtype == im.dtype == ar.dtype
    return re, im


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    kind = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(kind), b.view(kind))


def check_terms(got, X, prev, band, what, skip=0):
    """every = 1, first = 0 on a bit-identical route: each row is its term, bit for bit, from row `skip` on"""
    got = numpy_of(got)
    s = slice(band[0], band[0] + band[1])
    re, im = terms_of(X[:, s], None if prev is None else prev[s])
    assert got.shape == re.shape and got.real.dtype == re.dtype, (what, got.shape, re.shape, got.dtype)
    for name, g, t in (("re", got.real, re), ("im", got.imag, im)):
        g = np.ascontiguousarray(g)
        assert same_bits(g[skip:], t[skip:]), (what, name, int((g[skip:] != t[skip:]).sum()), float(np.abs(g[skip:] - t[skip:]).max()) if g[skip:].size else 0.0)
        if skip:
            assert np.all(g[:skip] == 0), (what, name, "the term against the zero row is not zero")


def check_sums(got, X, prev, n, every, first, band, exact, what, scale=1.0):
    """any grid: promise 3 per component, with promise 4 on top where the route is not bit-identical (scale: what its BAR is
    multiplied by on a route whose rows are held to another bar)"""
    got = numpy_of(got)
    s = slice(band[0], band[0] + band[1])
    re, im = terms_of(X[:n, s], None if prev is None else prev[s])
    w = windows(n, every, first)
    assert got.shape == (len(w), band[1]) and got.real.dtype == re.dtype, (what, got.shape, len(w), got.dtype)
    if not w:
        return
    hi = wide(re.dtype)
    u = hi(2.0 ** -24 if re.dtype == np.float32 else 2.0 ** -53)
    uw = hi(2.0 ** -53 if re.dtype == np.float32 else 2.0 ** -64)
    starts = [b for b, _ in w]
    L = np.array([e - b for b, e in w], dtype=hi)[:, None]
    xmax = hi(float((np.abs(X[:n, s]).astype(np.float64) ** 2).max()))
    for name, g, t in (("re", got.real, re), ("im", got.imag, im)):
        S = np.add.reduceat(t.astype(hi), starts, axis=0)
        T = np.add.reduceat(np.abs(t).astype(hi), starts, axis=0)
        bar = (L - 1) * u / (1 - (L - 1) * u) * T + L * uw * T
        if not exact:
            bar = bar + L * hi(BAR * scale) * xmax
        err = np.abs(g.astype(hi) - S)
        bad = err > bar
        assert not bad.any(), (what, name, int(bad.sum()), float((err / np.maximum(bar, np.finfo(hi).tiny)).max()))


def chunk_cursors(p, cursor0, m):
    """the cursor, modulo 2 m, at which every chunk of the plan's last call started (serial carries: chunk j starts at sample
    j * last_chunk_len); 0 -> the prologue took the accumulators themselves, else acc conj(fid)"""
    length, chunks = p.get_option("last_chunk_len"), p.get_option("last_chunks")
    return [(cursor0 + j * length) % (2 * m) for j in range(chunks)]


# ---------------------------------------------------------------------------------------------
# 1. parity at every = 1: the expression on consecutive rows, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_lag_sum_parity_one_chunk(combo, window):
    """calls shorter than 512 samples are one chunk: bit-identical for every type pair"""
    n = 300
    for i, m in enumerate((64, 1, 2, 3, 125)):
        x, X = rows_of(combo, window, m, n)
        bands = [(0, m)] + ([(1, m - 2)] if m >= 3 else [])
        with make(m, window, combo) as p:
            for j, band in enumerate(bands):
                p.reset()
                got = p.lag_sum(to_dev(x) if (i + j) % 2 else x, 1, 0, band=band)
                assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") == 1, (m, band)
                check_terms(got, X, None, band, (combo, window, m, band), skip=1)
            # band=None is the whole row
            p.reset()
            check_terms(p.lag_sum(x, 1), X, None, (0, m), (combo, window, m, "band=None"), skip=1)


@pytest.mark.parametrize("combo", O.COMBOS)
def test_lag_sum_parity_4096(combo):
    """several tiles; the band crosses the boundary between the first two"""
    m, n = 4096, 200
    x, X = rows_of(combo, "hann", m, n)
    with make(m, "hann", combo) as p:
        assert p.get_option("tiles") > 1
        per = p.get_option("interior") * p.get_option("bins_per_lane")          # bins a tile owns
        for i, band in enumerate([(per - 3, 7), (0, m), (m - 1, 1)]):
            p.reset()
            got = p.lag_sum(to_dev(x) if i % 2 else x, 1, 0, band=band)
            assert p.get_option("last_kernel") == 12
            check_terms(got, X, None, band, (combo, m, band), skip=1)


# ---------------------------------------------------------------------------------------------
# 2. exact carries, serial and relay form, several chunks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [0, None], ids=["serial", "default"])
@pytest.mark.parametrize("combo,opts", EXACT + [("f64f64", {"carry": 1})])
def test_lag_sum_exact_carries(combo, opts, chain):
    n = 6000
    for m in (64, 1000):
        x, X = rows_of(combo, "hann", m, n)
        band = (3, m - 5)
        with make(m, "hann", combo, **opts, **({} if chain is None else {"chain": chain})) as p:
            got = p.lag_sum(to_dev(x), 1, 0, band=band)
            assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1
            assert p.get_option("last_chain") == (0 if chain == 0 else 3), (combo, m, chain, p.get_option("last_chain"))
            check_terms(got, X, None, band, (combo, m, chain), skip=1)


# ---------------------------------------------------------------------------------------------
# 3. chunk boundaries: the row before a chunk's first sample comes from the chunk's carry-in
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT)
@pytest.mark.parametrize("chunk,ahead", [(256, 0), (200, 0), (256, 50), (200, 50)])
def test_lag_sum_chunk_boundaries(combo, opts, chunk, ahead):
    """m = 64: chunks of 256 samples from cursor 0 all start at cursor 0 (the prologue takes acc), chunks of 200 start inside
    blocks (acc conj(fid)), and a stream already 50 samples in starts chunk 0 inside a block as well"""
    m, n = 64, 2000
    x, X = rows_of(combo, "hann", m, ahead + n)
    for chain in (0, None):
        with make(m, "hann", combo, chunk=chunk, **opts, **({} if chain is None else {"chain": chain})) as p:
            if ahead:
                p.sdft(x[:ahead])
                assert p.state()[3] == ahead
            got = p.lag_sum(to_dev(x[ahead:]), 1, 0)
            assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1 and p.get_option("last_chunk_len") == chunk
            if chain == 0:                                   # (the relay form shifts its chunks to block boundaries of the cursor)
                assert p.get_option("last_chain") == 0
                cur = chunk_cursors(p, ahead, m)
                if chunk == 256 and ahead == 0:
                    assert all(c == 0 for c in cur), cur
                elif chunk == 256:
                    assert all(c == ahead for c in cur), cur
                else:
                    assert all(c != 0 for c in cur[1:]), cur
            check_terms(got, X[ahead:], X[ahead - 1] if ahead else None, (0, m), (combo, chunk, ahead, chain), skip=0 if ahead else 1)


# ---------------------------------------------------------------------------------------------
# 4. grids: windows inside chunks, cut by chunks, spanning several chunks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT + [("f64f32", {}), ("f64f64", {"carry": 1}), ("f32f64", {}), ("f64f64", {})],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "default" if isinstance(v, dict) else v)
def test_lag_sum_grids(combo, opts):
    m, n, band = 1000, 6000, (10, 300)
    x, X = rows_of(combo, "hann", m, n)
    exact = exact_combo(combo) or opts.get("carry") == 1
    dx = to_dev(x)
    with make(m, "hann", combo, **opts) as p:
        for i, (every, first) in enumerate(GRIDS):
            p.reset()
            got = p.lag_sum(dx if i % 2 else x, every, first, band=band)
            assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1
            if every >= 1024:
                assert every > p.get_option("last_chunk_len")                   # (a window over several chunks)
            if every == 1 and first == 0 and exact:
                check_terms(got, X, None, band, (combo, opts, every, first), skip=1)
            check_sums(got, X, None, n, every, first, band, exact, (combo, opts, every, first))


# ---------------------------------------------------------------------------------------------
# 5. streaming
# ---------------------------------------------------------------------------------------------
LENGTHS = [1, 99, 2000 - 100 + 1, 1, 100, 511, 512, 513]      # the fourth call starts one sample after the roll-over at 2000


@pytest.mark.parametrize("combo,opts", EXACT)
def test_lag_sum_streaming_terms(combo, opts):
    """every = 1: the calls' rows, one after the other, are one call's, bit for bit"""
    m, n, band = 1000, 6000, (10, 300)
    lengths = LENGTHS + [n - sum(LENGTHS)]
    assert sum(lengths[:3]) == 2 * m + 1 and lengths[3] == 1
    x, X = rows_of(combo, "hann", m, n)
    with make(m, "hann", combo, **opts) as p:
        parts, t = [], 0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            parts.append(numpy_of(p.lag_sum(to_dev(xs) if i % 3 == 1 else xs, 1, 0, band=band)))
            assert parts[-1].shape == (k, band[1])
            t += k
        got = np.concatenate(parts)
    check_terms(got, X, None, band, (combo, "streamed"), skip=1)
    with make(m, "hann", combo, **opts) as q:
        one = numpy_of(q.lag_sum(x, 1, 0, band=band))
    assert same_bits(got.real[1:], one.real[1:]) and same_bits(got.imag[1:], one.imag[1:]) and np.all(one[0] == 0)


@pytest.mark.parametrize("combo,opts", EXACT)
@pytest.mark.parametrize("every,first0", [(100, 37), (1024, 1023), (6000, 0)])
def test_lag_sum_streaming_grids(combo, opts, every, first0):
    """head rows added to the rows they complete: within promise 3 of the whole stream's windows (the host's additions are part of
    the ordered sum: a window of L terms in pieces is L - 1 additions at the most)"""
    m, n, band = 1000, 6000, (10, 300)
    lengths = LENGTHS + [n - sum(LENGTHS)]
    x, X = rows_of(combo, "hann", m, n)
    with make(m, "hann", combo, **opts) as p:
        rows, t, first = [], 0, first0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            d = numpy_of(p.lag_sum(to_dev(xs) if i % 3 == 1 else xs, every, first, band=band))
            assert d.shape == (power_sum_rows(k, every, first), band[1])
            if first > 0 and t > 0:
                rows[-1] = rows[-1] + d[0]              # the head completes the previous call's last row: the host adds the two
                d = d[1:]
            rows += list(d)
            first = every_next_first(k, every, first)
            t += k
        check_sums(np.array(rows), X, None, n, every, first0, band, True, (combo, every, first0, "streamed"))


@pytest.mark.parametrize("combo,opts", EXACT)
def test_lag_sum_between_other_entry_points(combo, opts):
    """sdft, lag_sum, power, lag_sum on one stream: the first term after a foreign call uses that call's last row"""
    m, band = 64, (0, 64)
    cuts = [0, 150, 450, 650, 1400]                          # (the last call has several chunks)
    x, X = rows_of(combo, "blackman", m, cuts[-1])
    with make(m, "blackman", combo, chunk=256, **opts) as p:
        assert np.array_equal(p.sdft(x[cuts[0]:cuts[1]]), X[cuts[0]:cuts[1]])
        a = p.lag_sum(x[cuts[1]:cuts[2]], 1, 0, band=band)
        assert p.get_option("last_kernel") == 12
        p.power(x[cuts[2]:cuts[3]], 1, 0)
        assert p.get_option("last_kernel") == 5
        b = p.lag_sum(to_dev(x[cuts[3]:cuts[4]]), 1, 0, band=band)
        assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1
    check_terms(a, X[cuts[1]:cuts[2]], X[cuts[1] - 1], band, (combo, "after sdft"))
    check_terms(b, X[cuts[3]:cuts[4]], X[cuts[3] - 1], band, (combo, "after power"))


# ---------------------------------------------------------------------------------------------
# 6. the state afterwards; an installed state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT)
@pytest.mark.parametrize("channels", [1, 3])
def test_lag_sum_leaves_the_state_of_sdft(combo, opts, channels):
    td = O.combo_types(combo)[0]
    m, n, band = 64, 2000, (30, 5)
    x = np.stack([signal(n, td, 40 + c) for c in range(channels)])
    x = x[0] if channels == 1 else x
    for device in (False, True):
        with make(m, "hann", combo, channels=channels, chunk=256, **opts) as p, make(m, "hann", combo, channels=channels, **opts) as q:
            p.lag_sum(to_dev(x) if device else x, 100, 37, band=band)
            assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1
            q.sdft(x)
            sp, sq = p.state(), q.state()
            assert sp[3] == sq[3] == n % (2 * m)
            for a, b in zip(sp[:3], sq[:3]):
                assert np.array_equal(a, b), (combo, channels, device)
            hop = x[..., :100]
            assert np.array_equal(p.sdft(hop), q.sdft(hop))


@pytest.mark.parametrize("combo,opts", EXACT)
@pytest.mark.parametrize("ahead", [128, 178], ids=["cursor-0", "inside-a-block"])
def test_lag_sum_after_set_state(combo, opts, ahead):
    """the state of a twin plan installed: the first term is the expression on the twin's last row"""
    m, n = 64, 700
    x, X = rows_of(combo, "hamming", m, ahead + n)
    with make(m, "hamming", combo, **opts) as q, make(m, "hamming", combo, chunk=256, **opts) as p:
        assert np.array_equal(q.sdft(x[:ahead]), X[:ahead])
        acc, fid, hist, cur = q.state()
        assert cur == ahead % (2 * m) and np.abs(acc).max() > 0
        p.set_state(acc, fid, hist, cur)
        for k in (100, n):                                   # one chunk, then several
            p.set_state(acc, fid, hist, cur)
            got = p.lag_sum(x[ahead:ahead + k], 1, 0)
            assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") == (k + 255) // 256
            check_terms(got, X[ahead:ahead + k], X[ahead - 1], (0, m), (combo, ahead, k))


# ---------------------------------------------------------------------------------------------
# 7. batched plans, host memory, async, repeatability
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT)
def test_lag_sum_batched_channels(combo, opts):
    """every channel by itself: its single-channel bits (at every = 1 always; on a coarser grid when both plans cut time alike)"""
    td = O.combo_types(combo)[0]
    ch, m, n, band = 3, 64, 2000, (17, 30)
    x = np.stack([signal(n, td, 100 + c) for c in range(ch)])
    for device in (False, True):
        for every, first in [(1, 0), (100, 37)]:
            with make(m, "blackman", combo, channels=ch, chunk=256, **opts) as p:
                got = numpy_of(p.lag_sum(to_dev(x) if device else x, every, first, band=band))
                assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1
                assert got.shape == (ch, power_sum_rows(n, every, first), band[1])
            for c in range(ch):
                with make(m, "blackman", combo, chunk=256, **opts) as q:
                    one = numpy_of(q.lag_sum(to_dev(x[c]) if device else x[c], every, first, band=band))
                assert same_bits(got[c].real, one.real) and same_bits(got[c].imag, one.imag), (combo, device, every, c)
                X = oracle_rows(O.best(m, "blackman", 1.0, combo), x[c])
                check_sums(got[c], X, None, n, every, first, band, True, (combo, device, every, c))


@pytest.mark.parametrize("combo,opts", EXACT)
def test_lag_sum_host_memory_in_segments(combo, opts):
    """host samples and host sums in three segments or more, and device samples with host sums, inside NaN sentinels: at every = 1
    the device-pointer call's bits; on a grid whose windows the segments cut, within promise 3 (the segments cut the windows
    elsewhere than the chunks of the one device call, and floating-point addition is not associative)"""
    fd = O.combo_types(combo)[1]
    m, n, band = 64, 2000, (17, 30)
    x, X = rows_of(combo, "hann", m, n)
    row = 2 * band[1] * np.dtype(fd).itemsize
    for every, first, stage in [(1, 0, 500 * row), (100, 37, 2 * row)]:
        rows = power_sum_rows(n, every, first)
        with make(m, "hann", combo, **opts) as d:
            dev = numpy_of(d.lag_sum(to_dev(x), every, first, band=band))
        with make(m, "hann", combo, stage_bytes=stage, **opts) as p:
            for xs in (x, to_dev(x)):
                p.reset()
                p.api.clear()
                arena = np.full(2 * (rows + 2) * band[1], np.nan, dtype=fd)
                out = arena[2 * band[1]:2 * (rows + 1) * band[1]]
                ptr = xs.data_ptr() if hasattr(xs, "data_ptr") else xs.ctypes.data
                assert p.api.sdft_lag_sum_n(p._p, n, C.c_void_p(ptr), every, first, band[0], band[1], C.c_void_p(out.ctypes.data)) == rows, p.api.last_error()
                p.synchronize()
                assert np.isnan(arena[:2 * band[1]]).all() and np.isnan(arena[2 * (rows + 1) * band[1]:]).all() and not np.isnan(out).any()
                got = out.view(dev.dtype).reshape(rows, band[1])
                if every == 1:
                    assert same_bits(got.real[1:], dev.real[1:]) and same_bits(got.imag[1:], dev.imag[1:]) and np.all(got[0] == 0)
                    check_terms(got, X, None, band, (combo, "host", hasattr(xs, "data_ptr")), skip=1)
                check_sums(got, X, None, n, every, first, band, True, (combo, every, first, "host", hasattr(xs, "data_ptr")))
            # host samples with device sums: a later segment's head is added on the device
            import torch
            p.reset()
            tarena = torch.full((2 * (rows + 2) * band[1],), float("nan"), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
            tout = tarena[2 * band[1]:2 * (rows + 1) * band[1]]
            assert p.api.sdft_lag_sum_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], C.c_void_p(tout.data_ptr())) == rows, p.api.last_error()
            p.synchronize()
            flat = tarena.cpu().numpy()
            assert np.isnan(flat[:2 * band[1]]).all() and np.isnan(flat[2 * (rows + 1) * band[1]:]).all()
            got = flat[2 * band[1]:2 * (rows + 1) * band[1]].view(dev.dtype).reshape(rows, band[1])
            assert not np.isnan(got).any()
            if every == 1:
                assert same_bits(got.real[1:], dev.real[1:]) and same_bits(got.imag[1:], dev.imag[1:]) and np.all(got[0] == 0)
            check_sums(got, X, None, n, every, first, band, True, (combo, every, first, "host samples, device sums"))


def test_lag_sum_async_device_pointers():
    m, n, band = 1000, 6000, (0, 256)
    x, X = rows_of("f32f64", "hann", m, n)
    with make(m, "hann", "f32f64", **{"async": 1}) as p:
        a = p.lag_sum(to_dev(x), 100, 37, band=band)
        p.synchronize()
        assert p.get_option("last_kernel") == 12
        check_sums(a, X, None, n, 100, 37, band, False, "async")


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_lag_sum_same_bits_on_every_run(combo):
    m, n = 1000, 6000
    x = rows_of(combo, "hann", m, n)[0]
    for device in (False, True):
        xs = to_dev(x) if device else x
        with make(m, "hann", combo) as p:
            for every, first in [(100, 37), (6000, 0)]:
                runs = []
                for _ in range(2):
                    p.reset()
                    d = numpy_of(p.lag_sum(xs, every, first))
                    assert p.get_option("last_chunks") > 1
                    runs.append(d)
                assert same_bits(runs[0].real, runs[1].real) and same_bits(runs[0].imag, runs[1].imag), (combo, device, every, first)


# ---------------------------------------------------------------------------------------------
# 8. no overrun, no hole, on an output offset by one sdft_fd_t
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo,opts", EXACT)
def test_lag_sum_guarded_misaligned_output(combo, opts, host):
    """sums carved from a guarded arena one sdft_fd_t off 16 bytes (so no complex number of a row is aligned to its own size); a
    band of 999 bins, windows of 7 samples after a head of 3, many of them cut by chunk boundaries"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 1000, 2000, 7, 3, (1, 999)
    x, X = rows_of(combo, "hann", m, n)
    rows = power_sum_rows(n, every, first)
    size = np.dtype(fd).itemsize
    with make(m, "hann", combo, **opts) as p:
        arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, 2 * band[1]), fd)))
        xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), np.array(x))
        out = arena.carve((rows, 2 * band[1]), fd, size, 16, name="sums")
        assert G.ptr_of(out) % 16 == size
        p.api.clear()
        got = p.api.sdft_lag_sum_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
        p.synchronize()
        assert got == rows, p.api.last_error()
        assert p.get_option("last_kernel") == 12 and p.get_option("last_chunks") > 1
        arena.check()
        assert G.view_unwritten(out) == 0
        assert np.array_equal(G.to_numpy(xv), x)
        flat = G.to_numpy(out)
        check_sums(flat[:, 0::2] + 1j * flat[:, 1::2], X, None, n, every, first, band, True, (combo, host))


# ---------------------------------------------------------------------------------------------
# 9. errors leave the state alone
# ---------------------------------------------------------------------------------------------
def test_lag_sum_errors():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as p:
        api = p.api
        p.lag_sum(x[:300], 7, 3)                            # (errors against a plan that is mid-stream)
        out = np.zeros((12, 2 * m), dtype=np.float32)
        before = p.state()
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"),              # every == 0
                   (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),             # nbins == 0
                   (100, 10, 0, 1, m, out.ctypes.data, "band"),              # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"),            # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL"),                         # rows > 0, sums NULL
                   (100, 10, 5000, 0, m, None, "NULL")]                      # first >= n: the head row is a row
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_lag_sum_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_lag_sum_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
        assert np.count_nonzero(out) == 0
        api.clear()
        assert api.sdft_lag_sum_n(None, 100, x.ctypes.data, 10, 0, 0, m, out.ctypes.data) == -1 and "NULL plan" in api.last_error()
        api.clear()
        # n == 0: no rows, nothing moves, sums may be NULL
        assert api.sdft_lag_sum_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.lag_sum(x[:10], 1, band=bad)
        with pytest.raises(ValueError):
            p.lag_sum(x[:10], 0)
        after = p.state()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]
        # the row counts of the C call
        for every, first in GRIDS:
            rows = power_sum_rows(1000, every, first)
            if rows <= out.shape[0]:
                p.reset()
                assert api.sdft_lag_sum_n(p._p, 1000, x.ctypes.data, every, first, 0, m, out.ctypes.data) == rows, (every, first)


# ---------------------------------------------------------------------------------------------
# 10. what the sums mean: the frequency of a sinusoid
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0.05, 0.113, 0.31])
def test_lag_sum_frequency_of_a_sinusoid(f):
    """f64f64, Hann, m = 64: row 1 of (every, first) = (500, 400) covers the samples 400 ... 899; at the bin of the largest |sum| the
    estimate is f to 1e-6 (the CPU oracle alone: 2.9e-9 at worst; a bin is 7.8e-3 wide).  A conjugate on the wrong side gives -f,
    a lag off by one and a swapped head row miss by far more than the bar."""
    m, n = 64, 1000
    x = np.sin(2 * np.pi * f * np.arange(n) + 0.3)
    with make(m, "hann", "f64f64") as p:
        sums = p.lag_sum(x, 500, 400)
        assert p.get_option("last_kernel") == 12
    assert sums.shape == (3, m) and sums.dtype == np.complex128
    k = int(np.argmax(np.abs(sums[1])))
    est = lag_frequency(sums)[1, k]
    print(f"f {f}: bin {k}, estimate off by {abs(est - f):.3e}")
    assert abs(est - f) <= 1e-6, (f, k, est)


# ---------------------------------------------------------------------------------------------
# 11. a plain C host: a stream in blocks, head rows added to the previous tails
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_lag_sum(tmp_path, hip_library, flags, combo):
    fd = O.combo_types(combo)[1]
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_lag_sum"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_lag_sum.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band = 1000, 6000, 100, 730, (0, 400)
    x, X = rows_of(combo, "hann", m, n)
    x.tofile(tmp_path / "x.raw")
    # the Python call in the same blocks: the bits the C host has to produce
    with make(m, "hann", combo) as p:
        rows, first = [], 0
        for t in range(0, n, block):
            k = min(block, n - t)
            d = p.lag_sum(x[t:t + k], every, first, band=band)
            if first > 0:
                rows[-1] = rows[-1] + d[0]
                d = d[1:]
            rows += list(d)
            first = every_next_first(k, every, first)
    want = np.array(rows)
    check_sums(want, X, None, n, every, 0, band, exact_combo(combo), (combo, "in blocks"))
    want.tofile(tmp_path / "want.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), str(tmp_path / "x.raw"), str(tmp_path / "want.raw"),
                        str(tmp_path / "s.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-LAG-SUM ok" in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fd).view(want.dtype).reshape(-1, band[1])
    assert same_bits(got.real, want.real) and same_bits(got.imag, want.imag)
