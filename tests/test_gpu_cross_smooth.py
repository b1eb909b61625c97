"""Smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n, SDFT.cross_smooth) on a real MI355X against the oracle.

The terms are formed by numpy in the FD dtype from the oracle's rows of the two channels of a pair (terms of
tests/test_gpu_cross_sum.py: four rounded products, one rounded sum, one rounded difference) and interleaved (re, im), so that a
pair's row is 2 * nbins real numbers -- the shape the library's own carry sees.  The recursion s = fl(fl(a * s) + fl(b * term))
runs on them elementwise, by numpy,
  * in the FD dtype (loop of tests/test_gpu_power_smooth.py) where bits are compared: calls of one time chunk, streams cut into
    such calls;
  * in np.float64 (FD float) or np.longdouble (FD double) (wide, below) where the bound of calls of several chunks is asserted:
    |got - s| <= 8 u M / (1 - a) per component, u = 2^-24 or 2^-53, M the running largest of the majorant
    m[t] = a m[t - 1] + b |term[t]| started at |state|.
On the route that is not bit-identical (FD double with default carries) the cross-spectrum call's term deviation, 2.1e-11 *
max|X_a| * max|X_b|, comes on top.

Three channels: channel 1 is half of channel 0 three samples late plus noise of its own (partly correlated), channel 2 is
independent; in the tests of the bound all carry a 40 dB burst over their middle fifth."""

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import SDFT, coherence, every_next_first, every_rows
from sdft_amd.signals import noise
from test_gpu_cross_sum import terms
from test_gpu_power import BAR, WINDOWS, make, signal, to_dev
from test_gpu_power_smooth import bit_opts, fd_of, host, loop, need_wide, wide_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYS = (0.0, 0.5, 0.9, 1.0 - 2.0 ** -10)
BOUND = 8.0
CH = 3
PAIRS = [(0, 1), (1, 0), (2, 2), (0, 1)]


def signals(td, n, seed, burst=False, channels=CH):
    x = np.empty((channels, n), dtype=td)
    x[0] = signal(n, td, seed)
    for c in range(1, channels):
        x[c] = signal(n, td, seed + 1000 * c)
    x[1] = np.roll(x[0], 3) * td(0.5) + noise(n, seed=seed + 7, dtype=td) * td(0.25)
    if burst:
        x[:, 2 * n // 5:3 * n // 5] *= td(100)
    return x


@functools.lru_cache(maxsize=3)
def rows_of(combo, window, m, n, cols=None, burst=False, channels=CH):
    """(samples (channels, n), the oracle's rows of every channel (channels, n, columns)); cols = (bin0, nbins) keeps those bins
    only.  Computed once, shared, never written"""
    td = O.combo_types(combo)[0]
    x = signals(td, n, m + 1, burst, channels)
    lo, nb = cols if cols else (0, m)
    X = None
    for c in range(channels):
        ref = O.best(m, window, 1.0, combo)
        for t in range(0, n, 2048):
            d = ref.sdft(x[c, t:t + 2048])
            if X is None:
                X = np.empty((channels, n, nb), dtype=d.dtype)
            X[c, t:t + 2048] = d[:, lo:lo + nb]
    x.setflags(write=False)
    X.setflags(write=False)
    return x, X


def pair_terms(X, pairs, band=None):
    """per pair the (n, 2 * nbins) real array of the terms, (re, im) interleaved, in the FD dtype"""
    out = []
    for a, b in pairs:
        A, B = (X[c] if band is None else X[c][:, band[0]:band[0] + band[1]] for c in (a, b))
        re, im = terms(A, B)
        t = np.empty((re.shape[0], 2 * re.shape[1]), dtype=re.dtype)
        t[:, 0::2], t[:, 1::2] = re, im
        out.append(t)
    return out


def flat(z):
    """a complex array (..., nbins) as the real array (..., 2 * nbins) the library stores"""
    z = np.ascontiguousarray(host(z))
    return z.view(z.real.dtype)


def wide(t, decay, state=None):
    """(n, numbers) of the exact recursion on the FD terms and the rounded coefficients, in the wide type; M, the running largest
    of the majorant m = a m + b |term| started at |state|; and u / (1 - a)"""
    from sdft_amd.sdft import smooth_coefficients
    fd, w = t.dtype, wide_of(t.dtype)
    a, b = (w(v) for v in smooth_coefficients(decay, fd))
    s = np.zeros(t.shape[1], dtype=w) if state is None else np.array(state, dtype=w)
    out, big = np.empty(t.shape, dtype=w), np.empty(t.shape, dtype=w)
    m = np.abs(s)
    top = m.copy()
    for i in range(t.shape[0]):
        tw = t[i].astype(w)
        s = a * s + b * tw
        m = a * m + b * np.abs(tw)
        top = np.maximum(top, m)
        out[i], big[i] = s, top
    u = w(2.0) ** (-24 if np.dtype(fd) == np.float32 else -53)
    return out, big, u / (w(1) - a)


def wide_of_pairs(T, pairs, decay, s0=None):
    """wide() per pair; a repeated pair shares the first one's reference"""
    seen, out = {}, []
    for p, pair in enumerate(pairs):
        if pair not in seen:
            seen[pair] = wide(T[p], decay, None if s0 is None else flat(s0[p]))
        out.append(seen[pair])
    return out


def sane(ref):
    """the reference is finite and its largest magnitude is a normal number"""
    ref = np.asarray(ref)
    assert ref.size and np.isfinite(ref).all()
    assert float(np.abs(ref).max()) >= float(np.finfo(np.float32 if ref.dtype == np.float32 else np.float64).tiny)


def same_bits(got, want, what):
    """got: complex or real from the library; want: the real (re, im) array"""
    got = flat(got) if np.iscomplexobj(host(got)) else host(got)
    sane(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(got.view(np.uint32 if got.dtype == np.float32 else np.uint64), want.view(np.uint32 if want.dtype == np.float32 else np.uint64)), \
        (what, int((got != want).sum()), float(np.abs(got - want).max()))


WORST = {}


def within_bound(got, ref, big, scale, what, extra=0.0):
    """|got - ref| <= BOUND * u M / (1 - a) (+ extra), number by number; -> the largest ratio err / (u M / (1 - a))"""
    got = flat(got) if np.iscomplexobj(host(got)) else host(got)
    sane(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = np.maximum(np.abs(got.astype(ref.dtype) - ref) - extra, 0)
    unit = scale * big
    assert not err[unit == 0].any(), what                   # (nothing has come in yet: s is exactly 0)
    ratio = float(np.divide(err, unit, out=np.zeros_like(err), where=unit > 0).max())
    key = np.dtype(got.dtype).name
    if ratio > WORST.get(key, 0.0):
        WORST[key] = ratio
        print(f"largest err / (u M / (1 - a)) so far, {key}: {ratio:.3f} at {what}")
    assert ratio <= BOUND, (what, f"largest err / (u M / (1 - a)) = {ratio:.3f}; so far, per FD type: {WORST}")
    return ratio


def plan_of(m, window, combo, pairs=PAIRS, channels=CH, **opts):
    p = make(m, window, combo, channels=channels, **opts)
    p.set_pairs([a for a, _ in pairs], [b for _, b in pairs])
    assert p.pairs == len(pairs)
    return p


def some_state(combo, pairs, nb, seed):
    """an incoming state (npairs, nb) complex: signed, of the size of the terms; consistent with the pair list -- (b, a) starts
    from the conjugate of (a, b), a repeat from the same numbers, (a, a) from a real number"""
    fdx = O.combo_types(combo)[2]
    rng = np.random.default_rng(seed)
    s = np.zeros((len(pairs), nb), dtype=fdx)
    seen = {}
    for i, (a, b) in enumerate(pairs):
        if (a, b) in seen:
            s[i] = s[seen[(a, b)]]
        elif (b, a) in seen:
            s[i] = np.conj(s[seen[(b, a)]])
        else:
            s[i] = ((rng.random(nb) - 0.5) * 60 + 1j * (rng.random(nb) - 0.5) * 60).astype(fdx)
            if a == b:
                s[i] = s[i].real + 0.25
        seen.setdefault((a, b), i)
    return s


def check_pair_relations(got, pairs, what, zero_imag=True):
    """promise 4 on one result (npairs, ..., nb) complex"""
    got = host(got)
    seen = {}
    for i, (a, b) in enumerate(pairs):
        if (a, b) in seen:
            assert np.array_equal(flat(got[i]).view(np.uint8), flat(got[seen[(a, b)]]).view(np.uint8)), (what, "repeat", i)
        if (b, a) in seen and a != b:
            j = seen[(b, a)]
            assert (got[i].real == got[j].real).all() and (got[i].imag == -got[j].imag).all(), (what, "conjugate", i, j)
        if a == b and zero_imag:
            assert (got[i].imag == 0).all() and not np.signbit(got[i].imag).any(), (what, "im of (a, a) is +0", i)
        seen.setdefault((a, b), i)


# ---------------------------------------------------------------------------------------------
# 1. one chunk: the sequential loop, bit for bit (promises 2 and 4)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_cross_smooth_one_chunk_is_the_loop_bit_for_bit(combo, window):
    fd = fd_of(combo)
    n, call = 300, 0
    for m in (1, 3, 64, 125):
        x, X = rows_of(combo, window, m, n)
        dx = to_dev(x)
        bands = [(0, m)] + ([(m // 3, m - m // 2)] if m > 1 else [])
        with plan_of(m, window, combo) as plan:
            for band in bands:
                T = pair_terms(X, PAIRS, band)
                for decay in DECAYS:
                    for given in (False, True):
                        s0 = some_state(combo, PAIRS, band[1], call) if given else None
                        want = [loop(T[i], decay, None if s0 is None else flat(s0[i])) for i in range(len(PAIRS))]
                        for every, first in [(1, 0), (7, 3), (n + 5, 0)]:
                            plan.reset()
                            call += 1
                            device = call % 2 == 1
                            state = None if s0 is None else (to_dev(s0) if (call // 2) % 2 else s0.copy())
                            got = plan.cross_smooth(dx if device else x, decay, every, first, bins=band, state=state)
                            what = (combo, window, m, band, decay, given, every, first)
                            assert plan.get_option("last_kernel") == 16 and plan.get_option("last_chunks") == 1, what
                            assert got.shape == (len(PAIRS), every_rows(n, every, first), band[1]), what
                            for i in range(len(PAIRS)):
                                same_bits(host(got)[i], want[i][0][first::every], what + (i,))
                                if given:
                                    same_bits(host(state)[i], want[i][1], what + (i, "state"))
                            check_pair_relations(got, PAIRS, what)
                            if given:
                                check_pair_relations(host(state), PAIRS, what + ("state",))
                    # (2, 2).re is the smoothed power call's value for channel 2 on the same plan, grid and re half of the state
                    plan.reset()
                    ps = np.zeros((CH, band[1]), dtype=fd)
                    ps[2] = s0[2].real
                    pw = plan.power_smooth(x, decay, 7, 3, bins=band, state=ps)
                    assert plan.get_option("last_chunks") == 1
                    assert np.array_equal(pw[2].view(np.uint8), np.ascontiguousarray(want[2][0][3::7, 0::2]).view(np.uint8)), (combo, window, m, band, decay)
                    assert np.array_equal(ps[2].view(np.uint8), np.ascontiguousarray(want[2][1][0::2]).view(np.uint8)), (combo, window, m, band, decay, "state")
            # bins=None is the whole row
            plan.reset()
            same_bits(plan.cross_smooth(x, 0.9, 7, 3)[0], loop(pair_terms(X, PAIRS[:1])[0], 0.9)[0][3::7], (combo, window, m, "bins=None"))


# ---------------------------------------------------------------------------------------------
# 2. several chunks: the bound (promise 6), on the bit-identical routes and with FD double's default carries
# ---------------------------------------------------------------------------------------------
def check_auto_against_power_smooth(plan, x, decay, every, first, band, s0, got, state, what, must_agree=False):
    """(a, a).re against power_smooth on the same plan, bit for bit, where both calls cut time alike"""
    i = [p for p, (a, b) in enumerate(PAIRS) if a == b][0]
    a = PAIRS[i][0]
    len_x = plan.get_option("last_chunk_len")
    plan.reset()
    ps = np.zeros((CH, band[1]), dtype=host(got).real.dtype)
    if s0 is not None:
        ps[a] = s0[i].real
    pw = host(plan.power_smooth(x, decay, every, first, bins=band, state=ps))
    alike = plan.get_option("last_chunk_len") == len_x
    assert alike or not must_agree, what
    if alike:
        assert np.array_equal(pw[a].view(np.uint8), np.ascontiguousarray(host(got)[i].real).view(np.uint8)), what + ("(a, a).re is power_smooth",)
        if state is not None:
            assert np.array_equal(ps[a].view(np.uint8), np.ascontiguousarray(host(state)[i].real).view(np.uint8)), what + ("(a, a).re state",)
    return alike


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("m", [1000, 1024])
def test_cross_smooth_several_chunks_within_the_bound(combo, m):
    """n = 6000: several chunks, a roll-over at 2N (at sample 2000 or 2048 and again later), a 40 dB burst; a band of 160 bins
    around the middle of the plan (the oracle's rows of three channels are kept for those bins only)"""
    need_wide(combo)
    n, band = 6000, (m // 2 - 81, 160)
    x, X = rows_of(combo, "hann", m, n, band, True)
    T = pair_terms(X, PAIRS)
    alike = 0
    with plan_of(m, "hann", combo, **bit_opts(combo)) as plan:
        for i, decay in enumerate(DECAYS[1:]):
            s0 = some_state(combo, PAIRS, band[1], i) if i % 2 else None
            refs = wide_of_pairs(T, PAIRS, decay, s0)
            for every, first in [(1, 0), (7, 3), (100, 37)][i:i + 2]:
                plan.reset()
                state = None if s0 is None else (to_dev(s0) if first else s0.copy())
                xs = to_dev(x) if every > 1 else x
                got = plan.cross_smooth(xs, decay, every, first, bins=band, state=state)
                what = (combo, m, decay, every, first)
                assert plan.get_option("last_kernel") == 16 and plan.get_option("last_chunks") > 1, what
                assert n > 2 * m and plan.get_option("last_chunk_len") < 2 * m          # (chunks begin on either side of a roll-over)
                for p, (ref, big, scale) in enumerate(refs):
                    within_bound(host(got)[p], ref[first::every], big[first::every], scale, what + (p,))
                    if s0 is not None:
                        within_bound(host(state)[p][None], ref[-1:], big[-1:], scale, what + (p, "state"))
                check_pair_relations(got, PAIRS, what)
                if every > 1:
                    alike += check_auto_against_power_smooth(plan, xs, decay, every, first, band, s0, got, state, what)
    print(f"(a, a).re compared with power_smooth bit for bit in {alike} calls of several chunks")


@pytest.mark.parametrize("combo", O.COMBOS)
def test_cross_smooth_forced_small_chunks_within_the_bound(combo):
    """n = 1500 at m = 64 with option "chunk" forced small: many chunks per bin, a partial band, the scan's batches of loads and
    its tail; the exact-carry routes' chunk shift when the plan is mid-stream"""
    need_wide(combo)
    m, n, band = 64, 1500, (5, 40)
    x, X = rows_of(combo, "blackman", m, n + 77, None, True)
    lead, x = x[:, :77], np.ascontiguousarray(x[:, 77:])     # (77 samples first: the cursor is odd, exact carries shift their chunks)
    T = [t[77:] for t in pair_terms(X, PAIRS, band)]
    for chunk in (128, 40):
        with plan_of(m, "blackman", combo, chunk=chunk, **bit_opts(combo)) as plan:
            for i, decay in enumerate(DECAYS[1:]):
                s0 = some_state(combo, PAIRS, band[1], 10 + i)
                plan.reset()
                plan.sdft(np.ascontiguousarray(lead))
                state = s0.copy()
                every, first = [(1, 0), (3, 2), (250, 249)][i]
                got = plan.cross_smooth(x, decay, every, first, bins=band, state=state)
                what = (combo, chunk, decay, every, first)
                assert plan.get_option("last_chunks") > 8, what
                for p, (ref, big, scale) in enumerate(wide_of_pairs(T, PAIRS, decay, s0)):
                    within_bound(got[p], ref[first::every], big[first::every], scale, what + (p,))
                    within_bound(state[p][None], ref[-1:], big[-1:], scale, what + (p, "state"))
                check_pair_relations(got, PAIRS, what)
                # (2, 2).re against power_smooth with the same forced chunks, from the same stream position
                len_x = plan.get_option("last_chunk_len")
                plan.reset()
                plan.sdft(np.ascontiguousarray(lead))
                ps = np.zeros((CH, band[1]), dtype=fd_of(combo))
                ps[2] = s0[2].real
                pw = plan.power_smooth(x, decay, every, first, bins=band, state=ps)
                assert plan.get_option("last_chunk_len") == len_x, what
                assert np.array_equal(pw[2].view(np.uint8), np.ascontiguousarray(got[2].real).view(np.uint8)), what + ("(2, 2).re is power_smooth",)
                assert np.array_equal(ps[2].view(np.uint8), np.ascontiguousarray(state[2].real).view(np.uint8)), what + ("(2, 2).re state",)


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_cross_smooth_band_across_a_tile_boundary(combo):
    """the hooks library's option "interior" cuts a small plan into several tiles: a band of two bins that lies across the first
    boundary, and the full band, in a call of several chunks; then option "interior" changed on the same plan"""
    need_wide(combo)
    m, n = 125, 1500
    x, X = rows_of(combo, "hann", m, n, None, True)
    with SDFT(m, "hann", 1.0, combo, CH, hooks=True) as plan:
        assert plan.get_option("test_hooks") == 1
        plan.set_pairs([a for a, _ in PAIRS], [b for _, b in PAIRS])
        for k, v in bit_opts(combo).items():
            plan.set_option(k, v)
        for interior in (31, 20):
            plan.set_option("interior", interior)
            per = plan.get_option("interior") * plan.get_option("bins_per_lane")
            assert plan.get_option("tiles") > 1 and per < m
            for band in [(per - 1, 2), (0, m)]:
                T = pair_terms(X, PAIRS, band)
                plan.reset()
                got = plan.cross_smooth(to_dev(x), 0.9, 7, 3, bins=band)
                assert plan.get_option("last_chunks") > 1 and plan.get_option("last_kernel") == 16
                for p, (ref, big, scale) in enumerate(wide_of_pairs(T, PAIRS, 0.9)):
                    within_bound(host(got)[p], ref[3::7], big[3::7], scale, (combo, interior, band, p))
            # ... and one chunk there: the loop's bits
            plan.reset()
            band = (per - 1, 2)
            T = pair_terms(X, PAIRS, band)
            got = plan.cross_smooth(x[:, :300], 0.9, 1, 0, bins=band)
            for p in range(len(PAIRS)):
                same_bits(got[p], loop(np.ascontiguousarray(T[p][:300]), 0.9)[0], (combo, interior, "one chunk", p))


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_cross_smooth_default_carries_within_the_bound_plus_the_term_deviation(combo):
    """FD double, fast carries: not the reference's rows bit for bit -- the cross-spectrum call's 2.1e-11 max|X_a| max|X_b| on top"""
    need_wide(combo)
    m, n, band = 1000, 6000, (419, 160)
    x, X = rows_of(combo, "hann", m, n, band, True)
    T = pair_terms(X, PAIRS)
    with plan_of(m, "hann", combo) as plan:
        got = plan.cross_smooth(to_dev(x), 0.9, 7, 3, bins=band)
        assert plan.get_option("last_chunks") > 1
        for p, (ref, big, scale) in enumerate(wide_of_pairs(T, PAIRS, 0.9)):
            a, b = PAIRS[p]
            extra = BAR * float(np.abs(X[a]).max()) * float(np.abs(X[b]).max())
            within_bound(host(got)[p], ref[3::7], big[3::7], scale, (combo, "default carries", p), extra=extra)


# ---------------------------------------------------------------------------------------------
# 3. decay 0 is the cross-spectrum call's every = 1 term on the grid's samples, on every route (promise 5)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_cross_smooth_decay_zero_is_the_cross_sum_term(combo):
    m, n, band = 1000, 6000, (451, 99)
    x = rows_of(combo, "hann", m, n, (419, 160), True)[0]
    for i, opts in enumerate([{}, dict(chunk=128), bit_opts(combo)]):
        with plan_of(m, "hann", combo, **opts) as plan, plan_of(m, "hann", combo, **opts) as twin:
            xs = to_dev(x) if i % 2 else x
            want = host(twin.cross_sum(xs, 1, 0, bins=band))
            assert want.shape == (len(PAIRS), n, band[1])
            for every, first in [(1, 0), (7, 3)]:
                plan.reset()
                state = some_state(combo, PAIRS, band[1], i)           # (forgotten at once: a == 0)
                got = host(plan.cross_smooth(xs, 0.0, every, first, bins=band, state=state))
                assert plan.get_option("last_chunks") > 1
                sane(flat(want))
                assert np.array_equal(got, want[:, first::every]), (combo, opts, every, first)
                # the state a decay of 0 leaves is the last sample's term
                assert np.array_equal(state, want[:, -1]), (combo, opts, every, first, "state")


# ---------------------------------------------------------------------------------------------
# 4. streaming (promise 3): one-chunk calls that pass state and first along have the loop's bits, wherever the cuts are
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_cross_smooth_streaming_in_one_chunk_calls_is_the_loop(combo):
    need_wide(combo)
    fdx = O.combo_types(combo)[2]
    m, n, band, decay = 64, 2000, (3, 50), float(np.exp(-1.0 / 40.0))
    x, X = rows_of(combo, "hamming", m, n, None, True)
    T = pair_terms(X, PAIRS, band)
    want = [loop(t, decay) for t in T]
    rng = np.random.default_rng(7)
    for every, first0 in [(1, 0), (7, 3), (450, 449)]:
        cuts, t = [], 0
        while t < n:
            k = min(int(rng.integers(1, 401)), n - t)
            cuts.append(k); t += k
        for device_state in (False, True):
            with plan_of(m, "hamming", combo) as plan:
                zero = np.zeros((len(PAIRS), band[1]), dtype=fdx)
                state = to_dev(zero) if device_state else zero
                rows, t, first = [[] for _ in PAIRS], 0, first0
                for i, k in enumerate(cuts):
                    xs = np.ascontiguousarray(x[:, t:t + k])
                    d = host(plan.cross_smooth(to_dev(xs) if i % 3 == 1 else xs, decay, every, first, bins=band, state=state))
                    assert plan.get_option("last_chunks") == 1
                    for p in range(len(PAIRS)):
                        rows[p] += list(d[p])
                    first = every_next_first(k, every, first)
                    t += k
                for p in range(len(PAIRS)):
                    same_bits(np.array(rows[p], dtype=fdx).reshape(-1, band[1]), want[p][0][first0::every], (combo, every, first0, device_state, len(cuts), p))
                    same_bits(host(state)[p], want[p][1], (combo, every, first0, device_state, "state", p))
    # the same signal as one long call of several chunks is within the bound of the loop's exact value
    with plan_of(m, "hamming", combo, **bit_opts(combo)) as plan:
        state = np.zeros((len(PAIRS), band[1]), dtype=fdx)
        got = plan.cross_smooth(x, decay, 7, 3, bins=band, state=state)
        assert plan.get_option("last_chunks") > 1
        for p in range(len(PAIRS)):
            ref, big, scale = wide(T[p], decay)
            within_bound(got[p], ref[3::7], big[3::7], scale, (combo, "one long call", p))
            within_bound(state[p][None], ref[-1:], big[-1:], scale, (combo, "one long call", "state", p))


# ---------------------------------------------------------------------------------------------
# 5. the stream state of every channel (promise 7), batched plans whose pairs share a channel, where state lives
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_cross_smooth_leaves_the_state_of_sdft(combo):
    """four channels, channel 3 in no pair, channel 0 in two: after the call the plan's state is a twin's after sdft_sdft_n of the
    same samples (one chunk, where both are the reference's bits), and sdft_sdft_n goes on bit for bit; for a long call the twin is
    cross_sum() at every = 1, the call that cuts time alike"""
    td = O.combo_types(combo)[0]
    m, ch = 125, 4
    pairs = [(0, 1), (2, 0), (1, 1)]
    x = signals(td, 6000, 9, channels=ch)
    hop = np.stack([noise(100, seed=12 + c, dtype=td) for c in range(ch)])
    for n, device in ((300, False), (300, True), (6000, True)):
        with plan_of(m, "hann", combo, pairs, ch) as plan, plan_of(m, "hann", combo, pairs, ch) as twin:
            xs = to_dev(x[:, :n]) if device else np.ascontiguousarray(x[:, :n])
            plan.cross_smooth(xs, 0.9, 7, 3, bins=(60, 5))               # (bins outside the band step too)
            if n == 300:
                twin.sdft(xs)
            else:
                twin.cross_sum(xs, 7, 3, bins=(60, 5))
                assert plan.get_option("last_chunks") == twin.get_option("last_chunks") > 1
                assert plan.get_option("last_chunk_len") == twin.get_option("last_chunk_len")
            for a, b in zip(plan.state()[:3], twin.state()[:3]):
                assert a.shape[0] == ch and np.array_equal(a, b), (combo, n, device)
            assert plan.state()[3] == twin.state()[3]
            dp, dq = plan.sdft(hop), twin.sdft(hop)
            assert np.array_equal(dp, dq)
            assert np.array_equal(plan.isdft(dp), twin.isdft(dq))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_cross_smooth_batched_pairs_that_share_a_channel(combo):
    need_wide(combo)
    m, band = 64, (17, 30)
    pairs = [(0, 1), (0, 2), (1, 2), (0, 0)]
    for n, opts in ((300, {}), (3000, bit_opts(combo))):
        x, X = rows_of(combo, "blackman", m, n, None, True)
        T = pair_terms(X, pairs, band)
        s0 = some_state(combo, pairs, band[1], 5)
        for device in (False, True):
            with plan_of(m, "blackman", combo, pairs, **opts) as plan:
                state = to_dev(s0) if device else s0.copy()
                got = host(plan.cross_smooth(to_dev(x) if device else x, 0.9, 7, 3, bins=band, state=state))
                assert got.shape == (len(pairs), every_rows(n, 7, 3), band[1]) and plan.get_option("last_kernel") == 16
                assert (plan.get_option("last_chunks") > 1) == (n > 512)
                for p in range(len(pairs)):
                    if n == 300:
                        want, end = loop(T[p], 0.9, flat(s0[p]))
                        same_bits(got[p], want[3::7], (combo, device, p))
                        same_bits(host(state)[p], end, (combo, device, p, "state"))
                    else:
                        ref, big, scale = wide(T[p], 0.9, flat(s0[p]))
                        within_bound(got[p], ref[3::7], big[3::7], scale, (combo, device, p))
                        within_bound(host(state)[p][None], ref[-1:], big[-1:], scale, (combo, device, p, "state"))
                # what a host does with the averages: the coherence of a channel with itself is 1
                c = coherence(got[3], got[3], got[3])
                assert np.isfinite(c).all() and np.allclose(c, 1.0, rtol=1e-5)


def test_cross_smooth_state_on_host_or_device_whatever_the_other_pointers_are():
    import torch
    combo, m, band, decay = "f32f32", 64, (3, 50), 0.9
    for n in (300, 1500):
        x, X = rows_of(combo, "hann", m, n)
        T = pair_terms(X, PAIRS, band)
        s0 = some_state(combo, PAIRS, band[1], 3)
        rows = every_rows(n, 7, 3)
        seen = []
        with plan_of(m, "hann", combo) as plan:
            for xd in (False, True):
                for od in (False, True):
                    for sd in (False, True):
                        plan.reset()
                        xs = to_dev(x) if xd else x
                        out = torch.zeros((len(PAIRS), rows, band[1]), dtype=torch.complex64, device="cuda") if od else np.zeros((len(PAIRS), rows, band[1]), dtype=np.complex64)
                        state = to_dev(s0) if sd else s0.copy()
                        ptr = lambda a: C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
                        got = plan.api.sdft_cross_smooth_n(plan._p, n, ptr(xs), 7, 3, band[0], band[1], decay, ptr(state), ptr(out))
                        plan.synchronize()
                        assert got == rows, plan.api.last_error()
                        seen.append((host(out).copy(), host(state).copy()))
            for p in range(len(PAIRS)):
                if n == 300:
                    want, end = loop(T[p], decay, flat(s0[p]))
                    same_bits(seen[0][0][p], want[3::7], "one chunk"); same_bits(seen[0][1][p], end, "one chunk, state")
                else:
                    # (host samples go in segments: the bits may differ between placements, each is within the bound)
                    ref, big, scale = wide(T[p], decay, flat(s0[p]))
                    for o, s in seen:
                        within_bound(o[p], ref[3::7], big[3::7], scale, "placements"); within_bound(s[p][None], ref[-1:], big[-1:], scale, "placements, state")
            if n == 300:
                assert all(np.array_equal(seen[0][0], o) and np.array_equal(seen[0][1], s) for o, s in seen[1:])


# ---------------------------------------------------------------------------------------------
# 6. host memory in segments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_cross_smooth_host_staging_in_segments(combo):
    """a small stage_bytes on host pointers: segments of one chunk each have the loop's bits (state travels between them on the
    device, the rows go through the call's own stage buffer pair by pair); longer segments are within the bound"""
    need_wide(combo)
    import torch
    fdx = O.combo_types(combo)[2]
    m, n, band, decay = 64, 2000, (3, 50), 0.9
    x, X = rows_of(combo, "hann", m, n, None, True)
    T = pair_terms(X, PAIRS, band)
    s0 = some_state(combo, PAIRS, band[1], 8)
    want = [loop(T[p], decay, flat(s0[p])) for p in range(len(PAIRS))]
    refs = wide_of_pairs(T, PAIRS, decay, s0)
    row = len(PAIRS) * band[1] * np.dtype(fdx).itemsize
    for every, first, stage, one_chunk in [(1, 0, 300 * row, True), (7, 3, 40 * row, True), (1, 0, 900 * row, False)]:
        with plan_of(m, "hann", combo, stage_bytes=stage, **bit_opts(combo)) as plan:
            rows = every_rows(n, every, first)
            plan.reset()
            state = s0.copy()
            got = plan.cross_smooth(x, decay, every, first, bins=band, state=state)
            what = (combo, stage, every, first)
            assert plan.get_option("last_segments") > 1, what
            if one_chunk:
                assert plan.get_option("last_chunks") == 1 and plan.get_option("last_chunk_len") < 512
            for p in range(len(PAIRS)):
                if one_chunk:
                    same_bits(got[p], want[p][0][first::every], what + (p,)); same_bits(state[p], want[p][1], what + (p, "state"))
                ref, big, scale = refs[p]
                within_bound(got[p], ref[first::every], big[first::every], scale, what + (p,))
                within_bound(state[p][None], ref[-1:], big[-1:], scale, what + (p, "state"))
            # host samples, device rows and state
            plan.reset()
            out = torch.zeros((len(PAIRS), rows, band[1]), dtype=getattr(torch, np.dtype(fdx).name), device="cuda")
            dstate = to_dev(s0)
            r = plan.api.sdft_cross_smooth_n(plan._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], decay, C.c_void_p(dstate.data_ptr()),
                                             C.c_void_p(out.data_ptr()))
            plan.synchronize()
            assert r == rows, plan.api.last_error()
            for p in range(len(PAIRS)):
                ref, big, scale = refs[p]
                within_bound(host(out)[p], ref[first::every], big[first::every], scale, what + ("device rows", p))
                within_bound(host(dstate)[p][None], ref[-1:], big[-1:], scale, what + ("device state", p))


# ---------------------------------------------------------------------------------------------
# 7. no overrun, no hole, at every alignment an element size allows: smooth and state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_side", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_cross_smooth_guarded_misaligned_buffers(combo, host_side):
    """smooth and state carved from a guarded arena at every residue modulo 16 the real element size allows, and at 16 mod 128; a
    band of 159 bins (an odd row length) in a call of several chunks, whose fix-up rewrites rows"""
    need_wide(combo)
    td, fd, fdx = O.combo_types(combo)
    m, n, every, first, cols = 1000, 2000, 7, 3, (419, 160)
    band = (cols[0] + 1, 159)
    x, X = rows_of(combo, "hann", m, 6000, cols, True)
    x = np.ascontiguousarray(x[:, :n])
    T = [t[:n] for t in pair_terms(X, PAIRS, (1, 159))]
    s0 = some_state(combo, PAIRS, band[1], 4)
    refs = wide_of_pairs(T, PAIRS, 0.9, s0)
    rows = every_rows(n, every, first)
    size = np.dtype(fd).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    np_ = len(PAIRS)
    with plan_of(m, "hann", combo, **bit_opts(combo)) as plan:
        for r, mod in places:
            arena = (G.HostArena if host_side else G.DeviceArena)(G.room(((CH, n), td), ((np_, rows, 2 * band[1]), fd), ((np_, 2 * band[1]), fd)))
            xv = G.put(arena.carve((CH, n), td, np.dtype(td).itemsize, 16, name="x"), x)
            out = arena.carve((np_, rows, 2 * band[1]), fd, r, mod, name="smooth")
            sv = G.put(arena.carve((np_, 2 * band[1]), fd, r, mod, name="state"), flat(s0))
            assert G.ptr_of(out) % mod == r and G.ptr_of(sv) % mod == r
            plan.reset()
            plan.api.clear()
            got = plan.api.sdft_cross_smooth_n(plan._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], 0.9, C.c_void_p(G.ptr_of(sv)),
                                               C.c_void_p(G.ptr_of(out)))
            plan.synchronize()
            assert got == rows, plan.api.last_error()
            assert plan.get_option("last_kernel") == 16 and plan.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            for p in range(np_):
                ref, big, scale = refs[p]
                within_bound(G.to_numpy(out)[p], ref[first::every], big[first::every], scale, (combo, host_side, r, mod, p))
                within_bound(G.to_numpy(sv)[p][None], ref[-1:], big[-1:], scale, (combo, host_side, r, mod, p, "state"))


# ---------------------------------------------------------------------------------------------
# 8. errors leave the stream state and the caller's state alone
# ---------------------------------------------------------------------------------------------
def test_cross_smooth_errors():
    combo, m = "f32f32", 64
    x = signals(np.float32, 3000, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo, channels=CH) as plan:
        api = plan.api
        out = np.zeros((len(PAIRS), 12, m), dtype=np.complex64)
        state = some_state(combo, PAIRS, m, 1)
        kept = state.copy()
        o, s = out.ctypes.data, state.ctypes.data
        # no pairs installed: refused, by the C call and by the Python call
        api.clear()
        assert api.sdft_cross_smooth_n(plan._p, 100, x.ctypes.data, 10, 0, 0, m, 0.5, s, o) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_cross_smooth_n" in err and "no pairs" in err, err
        api.clear()
        with pytest.raises(ValueError, match="set_pairs"):
            plan.cross_smooth(x[:, :10], 0.5)
        plan.set_pairs([a for a, _ in PAIRS], [b for _, b in PAIRS])
        plan.cross_smooth(np.ascontiguousarray(x[:, :300]), 0.5, 7, 3)      # (errors against a plan that is mid-stream)
        before = plan.state()
        refused = [(100, 0, 0, 0, m, 0.5, s, o, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, 0.5, s, o, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, 0.5, s, o, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, 0.5, s, o, "band"),
                   (100, 10, 0, 2, top, 0.5, s, o, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, 0, m, float("nan"), s, o, "decay"),
                   (100, 10, 0, 0, m, -0.25, s, o, "decay"),
                   (100, 10, 0, 0, m, 1.0, s, o, "decay"),
                   (100, 10, 0, 0, m, 1.0 - 2.0 ** -26, s, o, "decay"),   # rounds to 1 in FD float
                   (100, 10, 0, 0, m, float("inf"), s, o, "decay"),
                   (0, 10, 0, 0, m, 2.0, s, None, "decay"),               # ... even for a call without samples
                   (100, 10, 0, 0, m, 0.5, s, None, "NULL")]              # rows > 0, smooth NULL
        xb = np.ascontiguousarray(x[:, :100])
        for n, every, first, bin0, nb, decay, sp, op, word in refused:
            api.clear()
            assert api.sdft_cross_smooth_n(plan._p, n, xb.ctypes.data, every, first, bin0, nb, decay, sp, op) == -1, (every, bin0, nb, decay)
            err = api.last_error()
            assert err and "sdft_hip_sdft_cross_smooth_n" in err and word in err, err
            api.clear()
            after = plan.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb, decay)
            assert np.array_equal(state, kept), (every, bin0, nb, decay)
        assert np.count_nonzero(out) == 0
        # the decay's refusal message is the smoothed power call's
        message = "decay must be at least 0 and less than 1 after rounding to sdft_fd_t"
        api.clear()
        assert api.sdft_power_smooth_n(plan._p, 100, xb.ctypes.data, 10, 0, 0, m, 1.0, None, None) == -1 and message in api.last_error()
        api.clear()
        assert api.sdft_cross_smooth_n(plan._p, 100, xb.ctypes.data, 10, 0, 0, m, 1.0, s, o) == -1 and message in api.last_error()
        api.clear()
        # n == 0: no rows, nothing moves, smooth may be NULL, state stays
        assert api.sdft_cross_smooth_n(plan._p, 0, xb.ctypes.data, 10, 3, 0, m, 0.5, s, None) == 0 and api.last_error() is None
        assert plan.state()[3] == before[3] and np.array_equal(state, kept)
        # no row kept: smooth may be NULL, the state advances all the same
        assert api.sdft_cross_smooth_n(plan._p, 100, xb.ctypes.data, 10, 500, 0, m, 0.5, s, None) == 0 and api.last_error() is None
        assert not np.array_equal(state, kept) and plan.state()[3] != before[3]
        with plan_of(m, "hann", combo) as twin:
            twin.cross_smooth(np.ascontiguousarray(x[:, :300]), 0.5, 7, 3)
            want = kept.copy()
            twin.cross_smooth(xb, 0.5, 1, 0, state=want)
            assert np.array_equal(state, want)
        # the Python call refuses the same before it touches the plan
        for bad in (float("nan"), -0.25, 1.0):
            with pytest.raises(ValueError):
                plan.cross_smooth(xb, bad)
        with pytest.raises(ValueError):
            plan.cross_smooth(xb, 0.5, state=np.zeros((len(PAIRS), m - 1), dtype=np.complex64))


# ---------------------------------------------------------------------------------------------
# 9. the same bits on every run (promise 1)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_cross_smooth_same_bits_on_every_run(combo):
    m, n, band = 1000, 6000, (419, 160)
    x = rows_of(combo, "hann", m, n, band, True)[0]
    s0 = some_state(combo, PAIRS, band[1], 2)
    for device in (False, True):
        xs = to_dev(x) if device else x
        with plan_of(m, "hann", combo) as plan:
            for every, first in [(1, 0), (100, 37)]:
                runs = []
                for _ in range(3):
                    plan.reset()
                    state = to_dev(s0) if device else s0.copy()
                    d = plan.cross_smooth(xs, 0.9, every, first, bins=band, state=state)
                    assert plan.get_option("last_chunks") > 1
                    runs.append((flat(d).view(np.uint8), flat(state).view(np.uint8)))
                assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:]), (combo, device, every, first)


def test_cross_smooth_async_device_pointers():
    need_wide("f32f64")
    m, n, band = 1000, 6000, (419, 160)
    x, X = rows_of("f32f64", "hann", m, n, band, True)
    T = pair_terms(X, PAIRS)
    with plan_of(m, "hann", "f32f64", **{"async": 1}) as plan:
        state = to_dev(np.zeros((len(PAIRS), band[1]), dtype=np.complex128))
        got = plan.cross_smooth(to_dev(x), 0.9, 100, 37, bins=band, state=state)
        plan.synchronize()
        for p, (ref, big, scale) in enumerate(wide_of_pairs(T, PAIRS, 0.9)):
            a, b = PAIRS[p]
            extra = BAR * float(np.abs(X[a]).max()) * float(np.abs(X[b]).max())
            within_bound(host(got)[p], ref[37::100], big[37::100], scale, ("async", p), extra=extra)
            within_bound(host(state)[p][None], ref[-1:], big[-1:], scale, ("async, state", p), extra=extra)


# ---------------------------------------------------------------------------------------------
# 10. a plain C host and a C++ host: a stream in blocks, state passed from call to call
# ---------------------------------------------------------------------------------------------
def python_in_blocks(combo, m, x, pairs, every, block, band, decay):
    channels = x.shape[0]
    with plan_of(m, "hann", combo, pairs, channels) as plan:
        state = np.zeros((len(pairs), band[1]), dtype=O.combo_types(combo)[2])
        rows, first = [[] for _ in pairs], 0
        for t in range(0, x.shape[1], block):
            k = min(block, x.shape[1] - t)
            xs = np.ascontiguousarray(x[:, t:t + k]) if channels > 1 else np.ascontiguousarray(x[0, t:t + k])
            d = plan.cross_smooth(xs, decay, every, first, bins=band, state=state)
            for p in range(len(pairs)):
                rows[p] += list(d[p])
            first = every_next_first(k, every, first)
        return np.array(rows), state


@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_cross_smooth(tmp_path, hip_library, flags, combo):
    fdx = O.combo_types(combo)[2]
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_cross_smooth"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_cross_smooth.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band, decay = 64, 2000, 7, 330, (3, 50), 0.96875
    pairs = [(0, 1), (1, 0), (1, 1)]
    x, X = rows_of(combo, "hann", m, n, None, True)
    np.ascontiguousarray(x[:2]).tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), repr(decay), str(tmp_path / "x.raw"),
                        str(tmp_path / "s.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-CROSS-SMOOTH ok" in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fdx).reshape(len(pairs), -1, band[1])
    # blocks of 330 samples are one chunk each: the loop's bits over the whole signal, and the state's behind the last row
    T = pair_terms(X, pairs, band)
    for p in range(len(pairs)):
        want, end = loop(T[p], decay)
        same_bits(got[p, :-1], want[::every], ("C host", combo, p))
        same_bits(got[p, -1], end, ("C host", combo, p, "state"))
    rows, state = python_in_blocks(combo, m, x[:2], pairs, every, block, band, decay)
    assert np.array_equal(flat(got[:, :-1]).view(np.uint8), flat(rows).view(np.uint8)) and np.array_equal(flat(got[:, -1]).view(np.uint8), flat(state).view(np.uint8))


@pytest.mark.parametrize("t,f,combo", [("float", "double", "f32f64"), ("float", "float", "f32f32")])
def test_cpp_host_cross_smooth(tmp_path, hip_library, t, f, combo):
    fdx = O.combo_types(combo)[2]
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_cross_smooth_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", f"-DHOST_T={t}", f"-DHOST_F={f}", "-I", os.path.join(ROOT, "include", "cpp"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "host_cross_smooth.cpp"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band, decay = 64, 2000, 7, 330, (3, 50), 0.96875
    x, X = rows_of(combo, "hann", m, n, None, True)
    np.ascontiguousarray(x[2]).tofile(tmp_path / "x.raw")    # (a single-channel plan: the independent channel, the pair (0, 0) of it)
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), repr(decay), str(tmp_path / "x.raw"),
                        str(tmp_path / "s.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "CPP-CROSS-SMOOTH ok" in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fdx).reshape(-1, band[1])
    want, end = loop(pair_terms(X, [(2, 2)], band)[0], decay)
    same_bits(got[:-1], want[::every], ("C++ host", combo))
    same_bits(got[-1], end, ("C++ host", combo, "state"))
    rows, state = python_in_blocks(combo, m, x[2:3], [(0, 0)], every, block, band, decay)
    assert np.array_equal(flat(got[:-1]).view(np.uint8), flat(rows[0]).view(np.uint8)) and np.array_equal(flat(got[-1]).view(np.uint8), flat(state[0]).view(np.uint8))
