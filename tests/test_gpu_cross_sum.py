"""Pooled cross-spectrum analysis (sdft_hip_set_pairs, sdft_hip_sdft_cross_sum_n, SDFT.cross_sum) on a real MI355X against the
oracle.

Plans have 4 channels: sine_sweep(n) + 0.25 noise(n) with a seed per channel, channel 1 = 0.5 x channel 0 (a power of two: exact
through the whole recurrence, and every value stays normal), channel 3 in no pair.  The pairs are PAIRS.

The reference takes the oracle's rows of each channel, forms the terms with numpy in the FD dtype (numpy does not fuse)
    re = ar*br + ai*bi        im = ai*br - ar*bi
and sums them per window by a summation whose own error is far below u T for both FD dtypes: float64 prefix sums that carry
the exact error of every addition along (two-sum, as math.fsum does: hi + lo is the sum to better than 2^-100 of sum |term|), a
window being the difference of two prefixes; math.fsum itself checks a few windows and columns of every comparison.  (The wide
dtypes of tests/test_gpu_power_sum.py would do, but their per-window sums take many seconds for four channels and six pairs.)

The bar, per component, with L the window's length, u = 2^-24 (float) or 2^-53 (double), gamma_L = L u / (1 - L u) and
T = sum |term| over the window: gamma_L * T on the bit-identical routes (FD float, FD double with carry = 1, calls of one time
chunk); for FD double with default carries L * BAR * max|X_a| * max|X_b| comes on top (BAR = 2.1e-11 of tests/test_gpu_power.py,
the maxima over all rows of the call and the bins of its band).  The library promises gamma_(L-1); the step to gamma_L pays for the
reference's own rounding."""

import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import SdftHipError, every_next_first, power_sum_rows
from sdft_amd.signals import noise
from test_gpu_power import BAR, WINDOWS, bands_of, exact_combo, make, rel, signal, to_dev
from test_gpu_power_sum import GRIDS, windows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 4
PAIRS = [(0, 1), (1, 0), (2, 2), (0, 0), (0, 2), (0, 1)]
ALL_PAIRS = [(a, b) for a in range(CH) for b in range(CH)]
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the FD double reference needs an extended long double"


def signals(td, n, seed, channels=CH):
    """channel 1 is half of channel 0; every other channel c has a seed of its own, seed + 1000 (c - 1)"""
    x = np.empty((channels, n), dtype=td)
    x[0] = signal(n, td, seed)
    for c in range(1, channels):
        x[c] = x[0] * td(0.5) if c == 1 else signal(n, td, seed + 1000 * (c - 1))
    return x


def plan(m, window, combo, pairs=PAIRS, channels=CH, **opts):
    p = make(m, window, combo, channels=channels, **opts)
    p.set_pairs([a for a, _ in pairs], [b for _, b in pairs])
    assert p.pairs == len(pairs)
    return p


@functools.lru_cache(maxsize=2)
def rows_of(combo, window, m, n, cols=None, channels=CH):
    """(samples (channels, n), the oracle's rows of every channel (channels, n, columns)) of one shape; cols = (lo, hi) keeps those
    bins only.  Computed once, shared, never written"""
    td, fd, _ = O.combo_types(combo)
    x = signals(td, n, m, channels)
    lo, hi = cols if cols else (0, m)
    X = None
    for c in range(channels):
        ref = O.best(m, window, 1.0, combo)
        for t in range(0, n, 2048):
            d = ref.sdft(x[c, t:t + 2048])
            if X is None:
                X = np.empty((channels, n, hi - lo), dtype=d.dtype)
            X[c, t:t + 2048] = d[:, lo:hi]
    x.setflags(write=False)
    X.setflags(write=False)
    return x, X


def terms(A, B):
    """A conj(B) in the FD dtype: four rounded products, one rounded sum and one rounded difference, nothing fused"""
    re = A.real * B.real + A.imag * B.imag
    im = A.imag * B.real - A.real * B.imag
    return re, im


def prefix_sums(t):
    """(H, E): H[i] + E[i] is the sum of the rows t[:i] of the (n, k) array t, to far better than 2^-100 of sum |t[:i]|: H is the
    running float64 sum, E the sum of the exact errors of its additions (two-sum).  A window's sum is a difference of two rows."""
    t = t.astype(np.float64)                                # (exact for both FD dtypes)
    n, k = t.shape
    H = np.zeros((n + 1, k))
    np.cumsum(t, axis=0, out=H[1:])                         # in order, one rounded addition per row
    s, y = H[:-1], H[1:]
    assert np.array_equal(y, s + t)
    v = y - s
    E = np.zeros((n + 1, k))
    np.cumsum((s - (y - v)) + (t - v), axis=0, out=E[1:])   # the additions' exact errors (two-sum), summed
    return H, E


def window_sums(P, w, t):
    """(hi, lo): hi + lo is the sum of every window [b, e) of w from the prefix sums P of t, hi the float64 nearest to it (a
    window of one sample is that term)"""
    H, E = P
    b, e = np.array([b for b, _ in w]), np.array([e for _, e in w])
    hi, lo = np.empty((len(w), t.shape[1])), np.zeros((len(w), t.shape[1]))
    one = e - b == 1
    hi[one] = t[b[one]]
    b, e = b[~one], e[~one]
    y = H[e] - H[b]
    v = y - H[e]
    rest = ((H[e] - (y - v)) + (-H[b] - v)) + (E[e] - E[b])
    hi[~one] = y + rest
    lo[~one] = rest - (hi[~one] - y)
    return hi, lo


def reference(X, a, b, s, cache):
    """the terms of pair (a, b) over the band's columns s, their prefix sums and |terms|, once per (pair, band); the pair (b, a)
    of one that is there is its conjugate in value (numpy's products commute and x - y = -(y - x)), so re, the prefix sums and
    |terms| are taken from it.  The im terms are formed again all the same: where the difference is zero its SIGN is not that of
    -(y - x) -- (-0) - (+0) is -0 and (+0) - (-0) is +0 -- and at one bin every product of an im term is a zero of either sign
    (the rows are real), so the negated terms of (b, a) are not the expression's bits there"""
    if (a, b) not in cache:
        if (b, a) in cache:
            (re, pre, are), (_, (H, E), aim) = cache[(b, a)]
            cache[(a, b)] = [(re, pre, are), (terms(X[a][:, s], X[b][:, s])[1], (-H, -E), aim)]
        else:
            cache[(a, b)] = [(t, prefix_sums(t), np.abs(t).astype(np.float64)) for t in terms(X[a][:, s], X[b][:, s])]
    return cache[(a, b)]


def fsum_spot_check(t, w, hi, lo, rng):
    """the reference of the reference: math.fsum (exact, rounded once) on a few windows and columns"""
    for _ in range(3):
        r, k = int(rng.integers(len(w))), int(rng.integers(t.shape[1]))
        col = t[w[r][0]:w[r][1], k].astype(np.float64)
        exact = math.fsum(col)                               # (within half an ulp of the sum)
        assert abs((exact - hi[r, k]) - lo[r, k]) <= 2.0 ** -53 * abs(exact) + 2.0 ** -90 * float(np.abs(col).sum()), (r, k, exact, hi[r, k], lo[r, k])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_pairs(got, X, pairs, n, every, first, band, exact, what, col0=0, cache=None):
    """every pair and component of got (npairs, rows, nb) against the reference within the bar; on an exact route at
    every == 1, first == 0 bit for bit.  cache: a dict the caller keeps for one (X, band) over several grids"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    fd = X.real.dtype
    w = windows(n, every, first)
    assert got.shape == (len(pairs), len(w), band[1]) and got.dtype == X.dtype, (what, got.shape, got.dtype)
    if not w:
        return
    cache = {} if cache is None else cache
    rng = np.random.default_rng(every + first)
    s = slice(band[0] - col0, band[0] - col0 + band[1])
    u = 2.0 ** -24 if fd == np.float32 else 2.0 ** -53
    starts = [b for b, _ in w]
    L = np.array([e - b for b, e in w], dtype=np.float64)[:, None]
    gamma = L * u / (1 - L * u)
    if "amax" not in cache:
        cache["amax"] = [float(np.abs(X[c][:, s]).max()) for c in range(X.shape[0])]
    amax = cache["amax"]
    for i, (a, b) in enumerate(pairs):
        for comp, (t, P, mag) in zip((got[i].real, got[i].imag), reference(X, a, b, s, cache)):
            if exact and every == 1 and first == 0:
                assert same_bits(np.ascontiguousarray(comp), t), (what, (a, b), "not the expression's bits")
            hi, lo = window_sums(P, w, t)
            fsum_spot_check(t, w, hi, lo, rng)
            bar = gamma * np.add.reduceat(mag, starts, axis=0)
            if not exact:
                bar = bar + L * BAR * amax[a] * amax[b]
            err = np.abs((comp.astype(np.float64) - hi) - lo)      # (got - hi is exact wherever got is near the sum)
            bad = err > bar
            assert not bad.any(), (what, (a, b), int(bad.sum()), float((err / np.maximum(bar, np.finfo(np.float64).tiny)).max()))


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x grid x band
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_cross_sum_parity(combo, window):
    call = 0
    n = 6000                                    # several chunks, and a roll-over at 2N
    for m in (1, 2, 3, 5, 64, 125, 1000, 1024):
        x, X = rows_of(combo, window, m, n)
        dx = to_dev(x)
        with plan(m, window, combo) as p:
            bs = bands_of(m, p)
            # two of them: (50, 100), which crosses the first tile boundaries -- below 150 bins (1, m - 2), whose odd start puts the
            # float pairs off 8-byte alignment -- and the one wholly inside the last tile
            bands = list(dict.fromkeys([(50, 100) if (50, 100) in bs else bs[3] if len(bs) > 3 else bs[0], bs[-1]]))
            for band in bands:
                cache = {}                      # (the reference's terms and prefix sums of this band, shared by the grids)
                for every, first in GRIDS:
                    p.reset()
                    call += 1
                    got = p.cross_sum(dx if call % 2 else x, every, first, bins=band)
                    assert p.get_option("last_kernel") == 8, (m, every, first, band)
                    if m >= 1000:
                        assert p.get_option("last_chunks") > 1, (m, every, first, band)
                    check_pairs(got, X, PAIRS, n, every, first, band, exact_combo(combo), (combo, window, m, every, first, band), cache=cache)
            # bins=None is the whole row
            p.reset()
            check_pairs(p.cross_sum(x, 7, 6), X, PAIRS, n, 7, 6, (0, m), exact_combo(combo), (combo, window, m, "bins=None"))


def test_cross_sum_parity_4096():
    combo, m, n, cols = "f32f64", 4096, 10000, (4000, 4096)
    x, X = rows_of(combo, "hann", m, n, cols)
    with plan(m, "hann", combo) as p:
        for i, (every, first, band) in enumerate([(100, 37, (4000, 96)), (1024, 1023, (4033, 3)), (10000, 0, (4000, 96)), (7, 6, (4033, 3))]):
            p.reset()
            got = p.cross_sum(to_dev(x) if i % 2 else x, every, first, bins=band)
            assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
            check_pairs(got, X, PAIRS, n, every, first, band, False, (combo, m, every, first, band), col0=cols[0])


# ---------------------------------------------------------------------------------------------
# exact properties: auto-spectra, conjugates, repeats, the scaled channel; determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_cross_sum_exact_properties(combo):
    td = O.combo_types(combo)[0]
    n = 6000
    for m in (5, 125, 1000):
        x = signals(td, n, m)
        with plan(m, "hann", combo) as p, make(m, "hann", combo, channels=CH) as q:
            bs = bands_of(m, p)
            for i, (every, first) in enumerate([(1, 0), (100, 37), (6000, 0)]):
                band = bs[3] if i % 2 == 0 else bs[-1]
                xs = to_dev(x) if i % 2 else x
                p.reset()
                s = p.cross_sum(xs, every, first, bins=band)
                s = s.cpu().numpy() if i % 2 else s
                assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
                what = (combo, m, every, first, band)
                s01, s10, s22, s00, s02, s01b = s
                zero = np.zeros_like(s22.imag)
                # auto-spectra: im is +0; at every = 1 re is the power call's value
                assert same_bits(s22.imag.copy(), zero) and same_bits(s00.imag.copy(), zero), what
                assert (s22.real >= 0).all() and (s00.real >= 0).all(), what
                if every == 1:
                    q.reset()
                    pw = q.power(xs, 1, 0, bins=band)
                    pw = pw.cpu().numpy() if i % 2 else pw
                    # (FD double's default carries round alike only where the two calls cut time alike: here both do)
                    assert q.get_option("last_chunk_len") == p.get_option("last_chunk_len"), what
                    assert same_bits(s22.real.copy(), pw[2].copy()) and same_bits(s00.real.copy(), pw[0].copy()), what
                # (1, 0) is the conjugate of (0, 1); the repeated pair has the same bits.  (Channel 1 is half of channel 0, so both
                # imaginary parts are zero here: this pins re and the zeros; test_cross_sum_all_ordered_pairs checks the conjugates of
                # pairs of independent channels, whose imaginary parts are not zero.)
                assert same_bits(s10.real.copy(), s01.real.copy()) and np.array_equal(s10.imag, -s01.imag), what
                assert same_bits(s01b.copy(), s01.copy()), what
                # channel 1 = 0.5 x channel 0: (0, 1) is half of (0, 0), and real
                assert same_bits(s01.real.copy(), (s00.real * s00.real.dtype.type(0.5)).copy()) and same_bits(s01.imag.copy(), zero), what
                assert np.isfinite(s.real).all() and (np.abs(s00.real) >= np.finfo(s00.real.dtype).tiny).all(), what    # (all normal)
                # a pair of two independent channels is not real
                assert np.count_nonzero(s02.imag) > s02.imag.size // 2, what


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_cross_sum_is_the_expression_bit_for_bit_fd_double(combo):
    """promise (4) for FD double, whose default carries are not the reference's: with option carry = 1 (several chunks) and in a
    call shorter than 512 samples (one chunk, default carries) every value at every = 1, first = 0 -- pairs of two different
    channels included -- is the numpy expression on the oracle's rows bit for bit (check_pairs with exact = True asserts the bits),
    and pair (2, 2) is the power call's value on a twin plan with the same options"""
    n = 6000
    for m in (125, 1000):
        x, X = rows_of(combo, "hann", m, n)
        for opts, k in [(dict(carry=1), n), ({}, 500), (dict(carry=1), 500)]:
            with plan(m, "hann", combo, **opts) as p, make(m, "hann", combo, channels=CH, **opts) as q:
                bs = bands_of(m, p)
                for i, band in enumerate([bs[3], bs[-1]]):
                    xs = np.ascontiguousarray(x[:, :k])
                    xs = to_dev(xs) if i % 2 else xs
                    p.reset()
                    got = p.cross_sum(xs, 1, 0, bins=band)
                    got = got.cpu().numpy() if i % 2 else got
                    assert p.get_option("last_kernel") == 8 and (p.get_option("last_chunks") > 1) == (k == n), (combo, m, opts, k)
                    check_pairs(got, X[:, :k], PAIRS, k, 1, 0, band, True, (combo, m, opts, k, band))
                    q.reset()
                    pw = q.power(xs, 1, 0, bins=band)
                    pw = pw.cpu().numpy() if i % 2 else pw
                    assert same_bits(got[2].real.copy(), pw[2].copy()) and same_bits(got[3].real.copy(), pw[0].copy()), (combo, m, opts, k, band)


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_cross_sum_all_ordered_pairs(combo):
    """all 16 ordered pairs of the 4 channels: every (b, a) is the conjugate of (a, b) bit for bit, the values are right, and the
    state is the one sdft leaves (one writer per channel, however often it is named)"""
    m, n, every, first, band = 125, 6000, 100, 37, (1, 123)
    x, X = rows_of(combo, "hann", m, n)
    exact = exact_combo(combo)
    with plan(m, "hann", combo, pairs=ALL_PAIRS) as p, make(m, "hann", combo, channels=CH) as q:
        s = p.cross_sum(to_dev(x), every, first, bins=band).cpu().numpy()
        assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
        check_pairs(s, X, ALL_PAIRS, n, every, first, band, exact, (combo, "all pairs"))
        for a in range(CH):
            assert same_bits(s[a * CH + a].imag.copy(), np.zeros_like(s[0].imag)), (combo, a)
            for b in range(a + 1, CH):
                ab, ba = s[a * CH + b], s[b * CH + a]
                assert same_bits(ab.real.copy(), ba.real.copy()) and np.array_equal(ab.imag, -ba.imag), (combo, a, b)
        assert np.count_nonzero(s[0 * CH + 2].imag) > 0
        q.sdft(x)
        check_state(p, q, exact, (combo, "all pairs"))


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f32f64", {"carry": 1})])
def test_cross_sum_one_bin_both_orders_of_independent_channels(combo, opts):
    """A plan of one bin: the rows are real, so every product of an im term is a zero whose sign follows the signs of the two real
    parts, and so is the term.  With two independent channels named in both orders the im term of (0, 2) is -0 where that of (2, 0)
    is +0 and +0 where it is +0: not its negation.  The call forms each pair's expression on its own, as numpy does, bit for bit
    (every = 1, first = 0, exact carries, several chunks) -- what the sweep of tests/test_gpu_fuzz_grid.py found the reference of
    this file to get wrong (SDFT_FUZZ_OFFSET=1000, seed 33: it negated the cached terms of the other order)."""
    m, n, pairs = 1, 3000, [(2, 0), (0, 2), (2, 1), (1, 2)]
    x, X = rows_of(combo, "boxcar", m, n)
    im20, im02 = terms(X[2], X[0])[1], terms(X[0], X[2])[1]
    assert not np.any(im20) and not np.any(im02) and 0 < np.count_nonzero(np.signbit(im02)) < n         # zeros of both signs
    assert not same_bits(im02, -im20 + im20.dtype.type(0)) and not same_bits(im02, -im20)
    with plan(m, "boxcar", combo, pairs=pairs, **opts) as p:
        for i in range(2):
            p.reset()
            got = p.cross_sum(to_dev(x) if i else x, 1, 0)
            got = got.cpu().numpy() if i else got
            assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
            check_pairs(got, X, pairs, n, 1, 0, (0, 1), True, (combo, opts, "one bin, both orders", i))


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_cross_sum_same_bits_on_every_run(combo):
    m, n = 1000, 6000
    x = signals(O.combo_types(combo)[0], n, m)
    for device in (False, True):
        xs = to_dev(x) if device else x
        with plan(m, "hann", combo) as p:
            for every, first in [(100, 37), (6000, 0)]:
                runs = []
                for _ in range(3):
                    p.reset()
                    d = p.cross_sum(xs, every, first, bins=(1, 998))
                    assert p.get_option("last_chunks") > 1
                    runs.append(d.cpu().numpy() if device else d)
                assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), (combo, device, every, first)


# ---------------------------------------------------------------------------------------------
# streaming: uneven calls, head rows added to the previous tails; state; what follows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("every,first0", [(100, 37), (1024, 1023)])
def test_cross_sum_streaming(combo, every, first0):
    m, n, band = 125, 6000, (10, 100)
    lengths = [1, 99, 100, 511, 512, 513, 3000]
    lengths.append(n - sum(lengths))
    x, X = rows_of(combo, "hann", m, n)
    with plan(m, "hann", combo) as p:
        rows, t, first = None, 0, first0
        for i, k in enumerate(lengths):
            xs = np.ascontiguousarray(x[:, t:t + k])
            d = p.cross_sum(to_dev(xs) if i % 3 == 1 else xs, every, first, bins=band)
            d = d.cpu().numpy() if hasattr(d, "cpu") else d
            assert d.shape == (len(PAIRS), power_sum_rows(k, every, first), band[1])
            if first > 0 and t > 0:
                rows[:, -1] += d[:, 0]                   # the head completes the previous call's last row: the host adds the two
                d = d[:, 1:]
            rows = d.copy() if rows is None else np.concatenate([rows, d], axis=1)
            first = every_next_first(k, every, first)
            t += k
        # (the host's additions join pieces of one window: still at most L - 1 additions per row)
        check_pairs(rows, X, PAIRS, n, every, first0, band, exact_combo(combo), (combo, every, first0, "streamed"))


def check_state(p, q, exact, what):
    """the state of every channel of p against the twin q, which ran sdft over the same samples"""
    pa, pf, ph, pc = p.state()
    qa, qf, qh, qc = q.state()
    assert pc == qc and np.array_equal(ph, qh), what
    for c in range(pa.shape[0]):
        if exact:
            assert same_bits(pa[c].copy(), qa[c].copy()) and same_bits(pf[c].copy(), qf[c].copy()), (what, c)
        else:
            assert rel(pa[c], qa[c]) <= 1e-10 and rel(pf[c], qf[c]) <= 1e-10, (what, c, rel(pa[c], qa[c]), rel(pf[c], qf[c]))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_cross_sum_leaves_the_state_of_sdft(combo):
    """after the call the state of all four channels -- channel 3, which no pair names, included -- is the one sdft of the same
    samples leaves on a twin plan: bit for bit on the exact routes (FD float; FD double with carry = 1); with FD double's default
    carries the twin cuts time differently (its launch has 4 channels, this one 7 work items), so the tolerance is the one
    tests/test_gpu_power_sum.py uses where carries differ, 1e-10 of the largest value.  A following sdft and isdft continue."""
    td = O.combo_types(combo)[0]
    m, n = 125, 6000
    x = signals(td, n, m)
    hop = np.stack([noise(100, seed=12 + c, dtype=td) for c in range(CH)])
    eps = float(np.finfo(td).eps)
    for opts in ([{}, dict(carry=1)] if not exact_combo(combo) else [{}]):
        exact = exact_combo(combo) or "carry" in opts
        for device in (False, True):
            with plan(m, "hann", combo, **opts) as p, make(m, "hann", combo, channels=CH, **opts) as q:
                xs = to_dev(x) if device else x
                p.cross_sum(xs, 100, 37, bins=(10, 100))
                assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
                q.sdft(x)
                check_state(p, q, exact, (combo, opts, device))
                dp, dq = p.sdft(hop), q.sdft(hop)
                yp, yq = p.isdft(dp), q.isdft(dq)
                if exact:
                    assert np.array_equal(dp, dq) and np.array_equal(yp, yq)
                else:
                    assert rel(dp, dq) <= 1e-10, rel(dp, dq)
                    # (every bin within 1e-10 of the largest: the synthesis, a weighted mean of the bins, within that plus TD's rounding)
                    assert float(np.abs(yp - yq).max()) <= 1e-10 * float(np.abs(dq).max()) + 2 * eps * float(np.abs(yq).max())


def test_cross_sum_single_channel_plan():
    combo, m, n, band = "f32f32", 64, 3000, (3, 40)
    x = signal(n, np.float32, 7)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        p.set_pairs([0], [0])
        assert p.pairs == 1
        s = p.cross_sum(x, 1, 0, bins=band)
        assert s.shape == (1, n, band[1]) and p.get_option("last_kernel") == 8
        assert same_bits(s[0].real.copy(), q.power(x, 1, 0, bins=band)) and same_bits(s[0].imag.copy(), np.zeros((n, band[1]), np.float32))
        assert all(np.array_equal(a, b) for a, b in zip(p.state()[:3], q.state()[:3])) and p.state()[3] == q.state()[3]
        for a, b in ([0], [1]), ([1], [0]), ([0, 1], [0, 0]):
            with pytest.raises(SdftHipError, match="sdft_hip_set_pairs"):
                p.set_pairs(a, b)
            assert p.pairs == 1


# ---------------------------------------------------------------------------------------------
# forced routes, host staging, async
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(chunk=64), dict(chunk=8000), dict(carry=1), dict(carry=1, segments=2)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_cross_sum_forced_routes(opts):
    combo, m, n, band = "f32f64", 125, 6000, (1, 123)
    x, X = rows_of(combo, "hann", m, n)
    one_chunk = opts.get("chunk", 0) >= n
    with plan(m, "hann", combo, **opts) as p:
        # ((1, 0): on the exact routes -- carry = 1, one chunk -- every value is the numpy expression bit for bit, check_pairs)
        for every, first in [(1, 0), (100, 37), (6000, 0)]:
            p.reset()
            got = p.cross_sum(to_dev(x), every, first, bins=band)
            assert p.get_option("last_kernel") == 8
            assert (p.get_option("last_chunks") == 1) if one_chunk else (p.get_option("last_chunks") > 1)
            if opts.get("chunk") == 64:
                assert p.get_option("last_chunk_len") == 64
            if "segments" in opts:
                assert p.get_option("last_segments") == 2
            check_pairs(got, X, PAIRS, n, every, first, band, "carry" in opts or one_chunk, (opts, every, first))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_cross_sum_host_staging_in_segments(combo):
    """stage_bytes small enough for several segments: windows shorter than a segment, longer than one, and one over all of them;
    host samples with host and with device sums"""
    import torch
    fd = O.combo_types(combo)[1]
    m, n, band = 125, 6000, (10, 100)
    x, X = rows_of(combo, "hann", m, n)
    row = len(PAIRS) * 2 * band[1] * np.dtype(fd).itemsize
    for stage, grids in [(7 * row, [(100, 37), (100, 0)]), (2 * row, [(1024, 1023), (6000, 0), (700, 0)])]:
        with plan(m, "hann", combo, stage_bytes=stage) as p:
            for every, first in grids:
                rows = power_sum_rows(n, every, first)
                p.reset()
                check_pairs(p.cross_sum(x, every, first, bins=band), X, PAIRS, n, every, first, band, exact_combo(combo), (combo, stage, every, first, "host"))
                p.reset()
                out = torch.zeros((len(PAIRS), rows, band[1]), dtype=torch.complex64 if fd == np.float32 else torch.complex128, device="cuda")
                got = p.api.sdft_cross_sum_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], C.c_void_p(out.data_ptr()))
                p.synchronize()
                assert got == rows, p.api.last_error()
                check_pairs(out, X, PAIRS, n, every, first, band, exact_combo(combo), (combo, stage, every, first, "host samples, device sums"))


def test_cross_sum_async_device_pointers():
    combo, m, n, band = "f32f64", 125, 6000, (0, 125)
    x, X = rows_of(combo, "hann", m, n)
    with plan(m, "hann", combo, **{"async": 1}) as p:
        a = p.cross_sum(to_dev(x), 100, 37, bins=band)
        p.synchronize()
        check_pairs(a, X, PAIRS, n, 100, 37, band, False, "async")


# ---------------------------------------------------------------------------------------------
# errors leave the state and the installed list alone
# ---------------------------------------------------------------------------------------------
def test_cross_sum_errors():
    combo, m = "f32f32", 64
    x = signals(np.float32, 3000, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo, channels=CH) as p:
        api = p.api
        out = np.zeros((len(PAIRS), 12, m), dtype=np.complex64)
        # no pairs installed
        api.clear()
        assert api.sdft_cross_sum_n(p._p, 100, x.ctypes.data, 10, 0, 0, m, out.ctypes.data) == -1
        assert "sdft_hip_sdft_cross_sum_n" in api.last_error() and "pairs" in api.last_error()
        api.clear()
        with pytest.raises(ValueError):
            p.cross_sum(x[:, :10])
        p.set_pairs([a for a, _ in PAIRS], [b for _, b in PAIRS])
        p.cross_sum(np.ascontiguousarray(x[:, :300]), 7, 3)       # (errors against a plan that is mid-stream)
        before = p.state()
        # set_pairs refusals: the list stays
        pa = np.array([0, 1, 4], dtype=np.uint64)
        pb = np.array([0, 1, 2], dtype=np.uint64)
        for a, b, count, word in [(pa, pb, 3, "channel"), (pb, pa, 3, "channel"), (None, pb, 3, "NULL"), (pa, None, 3, "NULL"),
                                  (pb, pb, (1 << 31) + 1, "2^31"), (np.array([top], dtype=np.uint64), pb, 1, "channel")]:
            api.clear()
            assert api.set_pairs(p._p, count, None if a is None else a.ctypes.data, None if b is None else b.ctypes.data) == -1, word
            err = api.last_error()
            assert err and "sdft_hip_set_pairs" in err and word in err, err
            api.clear()
            assert p.pairs == len(PAIRS)
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, out.ctypes.data, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL"),                            # rows > 0, sums NULL
                   (100, 10, 5000, 0, m, None, "NULL")]                         # first >= n: the head row is a row
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_cross_sum_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_cross_sum_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
            assert p.pairs == len(PAIRS)
        assert np.count_nonzero(out) == 0
        # n == 0: no rows, nothing moves, sums may be NULL
        assert api.sdft_cross_sum_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.cross_sum(x[:, :10], bins=bad)
        with pytest.raises(ValueError):
            p.cross_sum(x[:, :10], every=0)
        # the list still works, and an empty one removes it
        assert p.cross_sum(np.ascontiguousarray(x[:, :100]), 10, 0).shape == (len(PAIRS), 10, m)
        p.set_pairs([], [])
        assert p.pairs == 0


# ---------------------------------------------------------------------------------------------
# no overrun, no hole, at every alignment of the buffers an element size allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_cross_sum_guarded_misaligned_buffers(combo, host):
    """sums carved from a guarded arena at every residue modulo 16 the element size of sdft_fd_t allows, and at 16 mod 128, the
    samples at an odd element; a band of 99 bins (an odd row length: consecutive rows change alignment), windows of 7 samples after
    a head of 3, many of them cut by chunk boundaries"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 125, 2000, 7, 3, (1, 99)
    x, X = rows_of(combo, "hann", m, 6000)
    x, X = np.ascontiguousarray(x[:, :n]), X[:, :n]
    rows = power_sum_rows(n, every, first)
    size = np.dtype(fd).itemsize
    tsize = np.dtype(td).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    with plan(m, "hann", combo) as p:
        for r, mod in places:
            arena = (G.HostArena if host else G.DeviceArena)(G.room(((CH, n), td), ((len(PAIRS), rows, 2 * band[1]), fd)))
            xv = G.put(arena.carve((CH, n), td, tsize, 16, name="x"), x)
            out = arena.carve((len(PAIRS), rows, 2 * band[1]), fd, r, mod, name="sums")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_cross_sum_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            s = G.to_numpy(out).reshape(len(PAIRS), rows, band[1], 2)
            s = np.ascontiguousarray(s).view(X.dtype)[..., 0]
            check_pairs(s, X, PAIRS, n, every, first, band, exact_combo(combo), (combo, host, r, mod))


# ---------------------------------------------------------------------------------------------
# a plain C host and the C++ facade
# ---------------------------------------------------------------------------------------------
def host_link(hip_library):
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    return ["-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]


def fnv1a(data: bytes) -> int:
    h = 1469598103934665603
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_cross_sum(tmp_path, hip_library, flags, combo):
    """tests/c/host_cross_sum.c: three channels, the pairs (0,0), (1,1), (0,1), (2,0), one call; its digest of the sums' bytes is
    the digest of the Python call's result on a plan of the same kind"""
    td = O.combo_types(combo)[0]
    exe = tmp_path / "host_cross_sum"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_cross_sum.c"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, ch, n, every, first, band = 64, 3, 1500, 100, 37, (3, 20)
    x = np.ascontiguousarray(signals(td, n, 3)[:ch])
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(ch), str(every), str(first), str(band[0]), str(band[1]), str(tmp_path / "x.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "C-HOST-CROSS-SUM ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    with plan(m, "hann", combo, pairs=[(0, 0), (1, 1), (0, 1), (2, 0)], channels=ch) as p:
        want = p.cross_sum(x, every, first, bins=band)
        assert p.get_option("last_chunks") > 1
    fields = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    assert int(fields["rows"]) == want.shape[1] and int(fields["digest"], 16) == fnv1a(want.tobytes()), (r.stdout, hex(fnv1a(want.tobytes())))
    assert abs(float(fields["coherence"]) - 1.0) < 1e-5           # channel 1 is half of channel 0: coherent in every bin


def test_cpp_facade_cross_sum(tmp_path, hip_library):
    """tests/cpp/host_cross_sum.cpp: sdft::SDFT<T, F>::set_pairs, pairs and cross_sum, compiled once"""
    exe = tmp_path / "host_cross_sum_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-DHOST_T=float", "-DHOST_F=double", "-I", os.path.join(ROOT, "include", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_cross_sum.cpp"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n = 125, 441
    signal(n, np.float32, 9).tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(tmp_path / "x.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CPP-CROSS-SUM ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
