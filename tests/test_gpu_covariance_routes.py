"""The array covariance call (sdft_hip_sdft_covariance_n, SDFT.covariance) on the windows, sizes and routes tests/test_gpu_covariance.py
leaves to its siblings' tests, on a real MI355X: the boxcar and hamming instantiations of the kernel, plans of 1, 2, 3 and 4096 bins,
the state on plans of several tiles with several groups, an array of 33 channels, forced carry routes on both FD types with the carry
form asserted, a state the host installed with a fid of its own per channel, device samples with host sums and segments bound by the
samples' bytes, tiles that change under an installed array, and all seven analysis entry points interleaved on a batched plan.

References and bars are those of tests/test_gpu_cross_sum.py: the oracle's rows (rows_of), numpy's unfused expression on them
(terms), check_pairs' bar -- gamma_L sum |term| on the bit-identical routes, L BAR max|X_a| max|X_b| on top for FD double's default
carries -- and, where only the library's order of addition defines the bits, the cross-spectrum call of a twin plan.  States are
compared bit for bit on the exact routes and to 1e-10 of the largest value elsewhere (check_state).  Element p(i, j) of an array
`chan` is the pair (chan[i], chan[j]) of check_pairs (pairs_of).

The carry form is the one tests/test_gpu_cross_sum_routes.py describes: no relay block divides 250, so a plan of 125 bins takes the
serial pass, a plan of 1000 bins the relay form; assert_route asserts the form every case ran."""

import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from sdft_amd.sdft import SDFT, power_sum_rows
from sdft_amd.signals import noise
from test_gpu_covariance import MIXED, N, array_plan, numpy_of, pairs_of, two_bands
from test_gpu_cross_sum import check_pairs, check_state, plan, rows_of, same_bits, signals
from test_gpu_cross_sum_routes import BANDS, DEFAULT_EXACT, ROUTE_CASES, assert_route, case_id, sentinel_sums
from test_gpu_filterbank import BOUNDED, geometry, run_interleaved, same_state
from test_gpu_power import WINDOWS, exact_combo, make, rel, to_dev
from test_gpu_power_sum import GRIDS

pytestmark = pytest.mark.gpu


def long_call(p, what, chunked=True):
    """forward_covariance_kernel, on several time chunks where time is meant to be cut"""
    assert p.get_option("last_kernel") == 9, (what, p.get_option("last_kernel"))
    if chunked:
        assert p.get_option("last_chunks") > 1, what


def first_boundary_band(p, m):
    """four bins across the first tile boundary, or None for a plan of one tile (test_cross_sum_pair_lists_and_their_writers)"""
    tiles, per = geometry(p)
    if tiles == 1:
        return None
    band = (per - 2, 4)
    assert band[0] + band[1] <= m and band[0] < per < band[0] + band[1]
    return band


# ---------------------------------------------------------------------------------------------
# 1. all four windows, the small sizes, 4096 bins
# ---------------------------------------------------------------------------------------------
def sizes_of(window):
    """boxcar (no halo) and hamming (a constant term) have not run at all; hann and blackman lack the plans narrower than a halo"""
    return (1, 2, 3, 5, 64, 125, 1000) if window in ("boxcar", "hamming") else (1, 2, 3)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("combo", O.COMBOS)
def test_covariance_parity_all_windows(combo, window):
    """n = 6000; 9 channels below 1000 bins, 5 there; per size an array with a padded last group and one of several groups; the
    bands of two_bands, below 4 bins the whole row; three of GRIDS per (array, band) in turn.  One bin: the halo cells are zero for
    ever (live[b]); 2 and 3 bins: the halo is wider than the row (reflect_bin)."""
    call = 0
    for m in sizes_of(window):
        channels, arrays = (9, [MIXED, list(range(9))]) if m < 1000 else (5, [list(range(5)), [3, 1]])
        x, X = rows_of(combo, window, m, N, None, channels)
        dx = to_dev(x)
        with make(m, window, combo, channels=channels) as p:
            if m == 1:
                assert p.size() == 1 and X.shape[2] == 1
            bands = two_bands(m, p) if m >= 4 else [(0, m)]
            caches = {band: {} for band in bands}
            for ai, chan in enumerate(arrays):
                p.set_array(chan)
                assert p.array_channels == len(chan)
                pairs = pairs_of(chan)
                for bi, band in enumerate(bands):
                    for every, first in GRIDS[(2 * ai + bi) % 3::3]:
                        p.reset()
                        call += 1
                        got = numpy_of(p.covariance(dx if call % 2 else x, every, first, bins=band))
                        what = (combo, window, m, chan, every, first, band)
                        long_call(p, what, chunked=m >= 1000)
                        if m == 1:
                            assert np.count_nonzero(got) > 0, what
                        check_pairs(got, X, pairs, N, every, first, band, exact_combo(combo), what, cache=caches[band])


def test_covariance_parity_4096():
    """the counterpart of test_cross_sum_parity_4096: many tiles, the band in the last of them"""
    combo, m, n, cols, chan = "f32f64", 4096, 10000, (4000, 4096), list(range(5))
    x, X = rows_of(combo, "hann", m, n, cols, 5)
    with array_plan(m, "hann", combo, chan, 5) as p:
        for i, (every, first, band) in enumerate([(100, 37, (4000, 96)), (1024, 1023, (4033, 3)), (10000, 0, (4000, 96)), (7, 6, (4033, 3))]):
            p.reset()
            got = p.covariance(to_dev(x) if i % 2 else x, every, first, bins=band)
            long_call(p, (m, every, first, band))
            check_pairs(got, X, pairs_of(chan), n, every, first, band, False, (combo, m, every, first, band), col0=cols[0])


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_covariance_group_sizes_on_the_other_windows(combo):
    """test_covariance_group_sizes_give_the_same_bits on the two windows it does not run: the candidates of the hooks build
    (option "array_group") return the bits of the product's choice"""
    td = O.combo_types(combo)[0]
    m, band = 125, (1, 123)
    x = signals(td, N, m, 9)
    opts = {} if exact_combo(combo) else dict(chunk=200)     # (FD double's default carries: the same chunks whatever the item count)
    call = 0
    for window in ("boxcar", "hamming"):
        for chan in ([2, 0, 1], list(range(9))):
            with array_plan(m, window, combo, chan, 9, **opts) as p:
                default = p.get_option("array_group")
                want = numpy_of(p.covariance(to_dev(x), 100, 37, bins=band))
                long_call(p, (combo, window, chan, "default"))
                before = p.state()
                for group in (1, 2, 4):
                    p.reset()
                    p.set_option("array_group", group)
                    assert p.get_option("array_group") == group and p.array_channels == len(chan)
                    call += 1
                    got = numpy_of(p.covariance(to_dev(x) if call % 2 else x, 100, 37, bins=band))
                    what = (combo, window, chan, group, default)
                    long_call(p, what)
                    if "chunk" in opts:
                        assert p.get_option("last_chunk_len") == opts["chunk"], what
                    assert same_bits(got, want), what
                    after = p.state()
                    assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], what


# ---------------------------------------------------------------------------------------------
# 2. the state on plans of several tiles
# ---------------------------------------------------------------------------------------------
class StateOf:
    """the state a plan had when this was made, for check_state"""

    def __init__(self, q):
        self.kept = q.state()

    def state(self):
        return self.kept


@pytest.mark.parametrize("window", ["hann", "blackman"])
@pytest.mark.parametrize("combo", O.COMBOS)
def test_covariance_state_on_many_tiles(combo, window):
    """1000 and 1024 bins, 5 channels: a band misses most tiles, and there a diagonal block steps its channels one after the other
    without windows and stores them (the kernel's `!emits` branch), while in the band's tiles it goes through the row loop.  Two
    diagonal blocks (5 channels), the same permuted, and an array that leaves three channels to advance-only items; a band of one
    bin in the first tile, one across the first tile boundary, one in the last tile.  The state of all channels is the one sdft
    leaves on a twin plan (check_state), a following sdft of 100 samples gives the twin's rows, and the values are right."""
    td = O.combo_types(combo)[0]
    hop = np.stack([noise(100, seed=12 + c, dtype=td) for c in range(5)])
    call = 0
    for m in (1000, 1024):
        x, X = rows_of(combo, window, m, N, None, 5)
        dx = to_dev(x)
        caches = {}
        for opts in ([{}, dict(carry=1)] if not exact_combo(combo) else [{}]):
            exact = exact_combo(combo) or "carry" in opts
            with make(m, window, combo, channels=5, **opts) as p, make(m, window, combo, channels=5, **opts) as q:
                tiles, per = geometry(p)
                one, across, last = (per // 2, 1), first_boundary_band(p, m), two_bands(m, p)[-1]
                assert tiles > 1 and one[0] // per == (one[0] + one[1] - 1) // per == 0
                assert last[0] // per == (last[0] + last[1] - 1) // per == tiles - 1
                q.sdft(dx)
                twin = StateOf(q)
                dq = q.sdft(hop)
                for chan in (list(range(5)), [4, 2, 0, 3, 1], [3, 1]):
                    p.set_array(chan)
                    assert p.array_channels == len(chan)
                    for band in (one, across, last):
                        what = (combo, window, m, opts, chan, band)
                        p.reset()
                        call += 1
                        got = p.covariance(dx if call % 2 else x, 100, 37, bins=band)
                        long_call(p, what)
                        check_state(p, twin, exact, what)
                        dp = p.sdft(hop)
                        if exact:
                            assert np.array_equal(dp, dq), what
                        else:
                            assert rel(dp, dq) <= 1e-10, (what, rel(dp, dq))
                        check_pairs(got, X, pairs_of(chan), N, 100, 37, band, exact, what, cache=caches.setdefault(band, {}))


# ---------------------------------------------------------------------------------------------
# 3. an array of 33 channels
# ---------------------------------------------------------------------------------------------
WIDE_ROUTES = [("f32f32", {}), ("f32f64", {"carry": 1}), ("f32f64", {})]


@pytest.mark.parametrize("combo,opts", WIDE_ROUTES, ids=case_id)
def test_covariance_wide_array(combo, opts):
    """64 bins, 40 plan channels, 3000 samples; the array a drawn permutation of 33 of them: with groups of 4 that is nine groups,
    the last of one channel -- 45 block items -- and 7 advance-only items behind them (the item index rest / launch_chunks and the
    output index p(i, j) for a large nch).  All 561 elements against the oracle's rows, and against cross_sum of a twin plan that
    has the same pairs as a list: the same bits, both calls cutting time alike (asserted).  The two calls count work items
    differently (52 against 568), so their own choices of a chunk length differ: on the exact routes the covariance call cuts as
    it chooses and the twin is given that length (option "chunk"), with FD double's default carries, whose bits depend on the
    cut, both are given 200.  The state of all 40 channels is the one sdft leaves."""
    m, ch, n, nch = 64, 40, 3000, 33
    exact = exact_combo(combo) or "carry" in opts
    forced = dict(opts) if exact else dict(opts, chunk=200)
    x, X = rows_of(combo, "hann", m, n, None, ch)
    chan = [int(c) for c in np.random.default_rng(33).permutation(ch)[:nch]]
    pairs = pairs_of(chan)
    assert len(set(chan)) == nch and len(pairs) == 561 and chan != sorted(chan)
    dx = to_dev(x)
    with array_plan(m, "hann", combo, chan, ch, **forced) as p, plan(m, "hann", combo, pairs=pairs, channels=ch, **forced) as t, \
            make(m, "hann", combo, channels=ch, **opts) as q:
        across = first_boundary_band(p, m)
        q.sdft(x)
        for i, (every, first, band) in enumerate([(7, 3, across or (1, m - 2)), (1, 0, across or (29, 4))]):
            what = (combo, opts, every, first, band)
            p.reset(); t.reset()
            xs = dx if i % 2 else x
            got = numpy_of(p.covariance(xs, every, first, bins=band))
            long_call(p, what)
            if exact:
                t.set_option("chunk", p.get_option("last_chunk_len"))
            want = numpy_of(t.cross_sum(xs, every, first, bins=band))
            assert t.get_option("last_kernel") == 8 and t.get_option("last_chunks") > 1, what
            assert p.get_option("last_chunk_len") == t.get_option("last_chunk_len"), (what, p.get_option("last_chunk_len"), t.get_option("last_chunk_len"))
            if "chunk" in forced:
                assert p.get_option("last_chunk_len") == forced["chunk"], what
            check_pairs(got, X, pairs, n, every, first, band, exact, what)
            assert same_bits(got, want), (what, int(np.count_nonzero(got.view(want.real.dtype) != want.view(want.real.dtype))))
            check_state(p, q, exact, what)


# ---------------------------------------------------------------------------------------------
# 4. forced routes on both FD types, the form asserted
# ---------------------------------------------------------------------------------------------
def routes_shape(m):
    return (9, MIXED) if m == 125 else (5, list(range(5)))


@pytest.mark.parametrize("combo,m,opts", ROUTE_CASES, ids=case_id)
def test_covariance_forced_routes_both_fd_types(combo, m, opts):
    """test_cross_sum_forced_routes_both_fd_types for the covariance call: device samples, three grids, the route asserted with
    the carry form (the relay form hands `load` a fid from a table for every slot of a group, the serial form each channel's own
    seed).  On the exact routes at (1, 0) the bits of a plan on the default exact route."""
    band = BANDS[m]
    channels, chan = routes_shape(m)
    pairs = pairs_of(chan)
    x, X = rows_of(combo, "hann", m, N, None, channels)
    dx = to_dev(x)
    exact = exact_combo(combo) or "carry" in opts
    with array_plan(m, "hann", combo, chan, channels, **opts) as p, make(m, "hann", combo, channels=channels, **opts) as q, \
            array_plan(m, "hann", combo, chan, channels, **DEFAULT_EXACT[combo]) as d:
        q.sdft(dx)
        cache = {}
        for every, first in [(1, 0), (100, 37), (N, 0)]:
            what = (combo, m, opts, every, first)
            p.reset()
            got = p.covariance(dx, every, first, bins=band)
            assert_route(p, opts, exact, m, what, kernel=9)
            check_pairs(got, X, pairs, N, every, first, band, exact, what, cache=cache)
            check_state(p, q, exact, what)
            if exact and (every, first) == (1, 0):
                d.reset()
                assert same_bits(numpy_of(got), numpy_of(d.covariance(dx, every, first, bins=band))), what
                assert_route(d, DEFAULT_EXACT[combo], True, m, (what, "default exact route"), kernel=9)


@pytest.mark.parametrize("every,first", [(1, 0), (100, 37)])
def test_covariance_relay_form_from_a_cursor_inside_a_block(every, first):
    """FD float, 1000 bins: a first call of 700 samples leaves the cursor at a multiple of no block length, so the chunks of the
    long call on the other 5300 are shifted to begin on block boundaries (chunk_shift != 0)"""
    combo, m, k, chan = "f32f32", 1000, 700, list(range(5))
    band = BANDS[m]
    x, X = rows_of(combo, "hann", m, N, None, 5)
    with array_plan(m, "hann", combo, chan, 5) as p, make(m, "hann", combo, channels=5) as q:
        p.power(np.ascontiguousarray(x[:, :k]), 7, 3, bins=(0, m))
        assert p.get_option("cursor") == k and all(k % block for block in (8, 16, 32, 64, 128))
        got = p.covariance(to_dev(x[:, k:]), every, first, bins=band)
        assert_route(p, {}, True, m, (every, first), kernel=9)
        assert p.get_option("last_chain") == 3
        check_pairs(got, X[:, k:], pairs_of(chan), N - k, every, first, band, True, ("from cursor 700", every, first))
        q.sdft(np.ascontiguousarray(x[:, :k])); q.sdft(to_dev(x[:, k:]))
        check_state(p, q, True, ("from cursor 700", every, first))


# ---------------------------------------------------------------------------------------------
# 5. a state installed by the host, a fid of its own per channel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", BOUNDED, ids=case_id)
def test_covariance_after_a_state_with_a_fid_of_its_own_per_channel(combo, opts):
    """test_cross_sum_after_a_state_with_a_fid_of_its_own_per_channel for the covariance call: the host installs a state in which
    channel c's fid is (1 + c / 1024) times the one sdft left, so the serial form has to hand every slot of a group -- up to 2 G
    channels per wave, padded slots included -- its own channel's seed.  The reference is numpy's expression on the rows a twin
    plan's sdft gives from the same installed state, and the twin's state afterwards, bit for bit."""
    m, k, ch = 125, 1500, 9
    band = BANDS[m]
    cols = slice(band[0], band[0] + band[1])
    x, X = rows_of(combo, "hann", m, N, None, ch)
    head, tail = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
    with make(m, "hann", combo, channels=ch, **opts) as t:
        t.sdft(head)
        acc, fid, hist, cursor = t.state()
        fid = fid * (1 + np.arange(ch) / 1024).astype(fid.real.dtype)[:, None]
        assert fid.dtype == X.dtype
        t.set_state(acc, fid, hist, cursor)
        rows = t.sdft(tail)
        assert t.get_option("last_chain") == 0 and t.get_option("last_chunks") > 1
        assert np.array_equal(rows[0], X[0, k:]) and not np.array_equal(rows[2][:, cols], X[2, k:, cols])     # (the fid matters)
        call = 0
        for chan in (MIXED, list(range(9))):
            assert all(not np.array_equal(fid[a], fid[b]) for a in chan for b in chan if a < b)
            for every, first in [(1, 0), (100, 37)]:
                what = (combo, "fid per channel", chan, every, first)
                with array_plan(m, "hann", combo, chan, ch, **opts) as r:
                    r.set_state(acc, fid, hist, cursor)
                    call += 1
                    got = numpy_of(r.covariance(to_dev(tail) if call % 2 else tail, every, first, bins=band))
                    assert_route(r, dict(opts, chain=0), True, m, what, kernel=9)
                    assert r.get_option("last_chain") == 0, what
                    check_pairs(got, rows, pairs_of(chan), N - k, every, first, band, True, what)      # ((1, 0): the expression's bits)
                    assert same_state(r, t), what


# ---------------------------------------------------------------------------------------------
# 6. device samples with host sums; segments bound by the samples' bytes
# ---------------------------------------------------------------------------------------------
def raw_covariance(p, x, n, every, first, band, cov):
    ptr = lambda a: C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    p.api.clear()
    got = p.api.sdft_covariance_n(p._p, n, ptr(x), every, first, band[0], band[1], ptr(cov))
    p.synchronize()
    assert got == power_sum_rows(n, every, first), (got, p.api.last_error())
    assert p.get_option("last_kernel") == 9


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_covariance_staging_device_samples_host_sums_and_sample_bound_segments(combo):
    """the counterpart of test_cross_sum_staging_device_samples_host_sums_and_sample_bound_segments, whose host code this call has
    a copy of: stage_bytes of 7 and of 2 rows of the triangle with device samples and host sums (per-element copies out of the
    device scratch, head rows added on the host), stage_bytes of 700 samples of 9 channels with host samples into host and into
    device sums.  The output is NaN beforehand and has none afterwards; the values are within the bar, on FD float at (1, 0) they
    are the bits of the unstaged device-to-device call, and the state is that call's."""
    td, fd, _ = O.combo_types(combo)
    m, band, chan, ch = 125, (10, 100), [2, 0, 1], 9
    exact = exact_combo(combo)
    pairs = pairs_of(chan)
    x, X = rows_of(combo, "hann", m, N, None, ch)
    dx = to_dev(x)
    row = len(pairs) * 2 * band[1] * np.dtype(fd).itemsize
    one = [(1, 0)] if exact else []
    runs = [("device samples, host sums", 7 * row, dx, False, [(100, 37), (100, 0)] + one),
            ("device samples, host sums", 2 * row, dx, False, [(1024, 1023), (N, 0), (700, 0)]),
            ("host samples, host sums", 700 * ch * np.dtype(td).itemsize, x, False, [(100, 37), (700, 699), (N, 0)]),
            ("host samples, device sums", 700 * ch * np.dtype(td).itemsize, x, True, [(100, 37), (700, 699)] + one)]
    with array_plan(m, "hann", combo, chan, ch) as q:
        for kind, stage, xs, device_sums, grids in runs:
            with array_plan(m, "hann", combo, chan, ch, stage_bytes=stage) as p:
                for every, first in grids:
                    what = (combo, kind, stage, every, first)
                    rows = power_sum_rows(N, every, first)
                    q.reset()
                    want = numpy_of(q.covariance(dx, every, first, bins=band))
                    long_call(q, (what, "unstaged"))
                    p.reset()
                    out = sentinel_sums(fd, rows, band[1], device_sums, npairs=len(pairs))
                    raw_covariance(p, xs, N, every, first, band, out)
                    out = numpy_of(out)
                    assert out.shape == want.shape and not np.isnan(out.real).any() and not np.isnan(out.imag).any(), (what, "an element was left unwritten")
                    check_pairs(out, X, pairs, N, every, first, band, exact, what)
                    if exact and (every, first) == (1, 0):
                        assert same_bits(out, want), what
                    assert same_state(p, q) if exact else p.state()[3] == q.state()[3], what


# ---------------------------------------------------------------------------------------------
# 7. option "interior" changes the tiles under an installed array
# ---------------------------------------------------------------------------------------------
TILES_ARRAY = [4, 2, 0, 3, 1]
TILES_PAIRS = [(3, 3), (2, 0)]


def hooked_array(combo, opts, hooks=True):
    p = SDFT(1024, "hann", 1.0, combo, channels=5, hooks=hooks)
    for k, v in opts.items():
        p.set_option(k, v)
    p.set_array(TILES_ARRAY)
    assert p.array_channels == len(TILES_ARRAY)
    return p


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {})], ids=case_id)
def test_covariance_when_the_tiles_change_under_an_installed_array(combo, opts):
    """the counterpart of test_cross_sum_when_the_tiles_change_under_an_installed_list: the tiles' test against the band follows
    the tiles of the call, the array stays installed; and an array installed in the product library moves with the plan to the
    hooks library (SDFT.set_option replays it, and a pair list beside it) together with the state"""
    m, every, first, band, other = 1024, 7, 6, (50, 100), 62
    exact = exact_combo(combo) or "carry" in opts
    pairs = pairs_of(TILES_ARRAY)
    x, X = rows_of(combo, "hann", m, N, None, 5)
    with hooked_array(combo, opts) as p:
        assert p.get_option("test_hooks") == 1
        tiles0, interior0 = p.get_option("tiles"), p.get_option("interior")
        assert interior0 != other
        outs, cache = [], {}
        for step, lanes in enumerate((interior0, other, interior0)):
            p.set_option("interior", lanes)
            assert p.get_option("interior") == lanes and (p.get_option("tiles") != tiles0) == (lanes != interior0)
            p.reset()
            outs.append(numpy_of(p.covariance(to_dev(x) if step % 2 else x, every, first, bins=band)))
            assert p.array_channels == len(TILES_ARRAY)
            long_call(p, (combo, "interior", lanes))
            check_pairs(outs[-1], X, pairs, N, every, first, band, exact, (combo, "interior", lanes), cache=cache)
        assert same_bits(outs[0], outs[2]), combo
    # installed in the product library, a call, then an option only the hooks library knows
    k = 700
    head, tail = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
    with hooked_array(combo, opts, hooks=False) as p, hooked_array(combo, opts, hooks=False) as q:
        assert p.get_option("test_hooks") == 0
        p.set_pairs([a for a, _ in TILES_PAIRS], [b for _, b in TILES_PAIRS])
        first_part = p.covariance(head, every, first, bins=band)
        assert same_bits(first_part, q.covariance(head, every, first, bins=band))
        assert p.get_option("last_kernel") == 9 and q.get_option("last_kernel") == 9
        p.set_option("interior", other)
        assert p.get_option("test_hooks") == 1 and p.get_option("interior") == other and p.get_option("tiles") != tiles0
        assert q.get_option("test_hooks") == 0 and q.get_option("tiles") == tiles0
        assert p.array_channels == len(TILES_ARRAY) and p.pairs == len(TILES_PAIRS)
        assert p.state()[3] == k and (same_state(p, q) if exact else p.state()[3] == q.state()[3])
        got = numpy_of(p.covariance(to_dev(tail), every, first, bins=band))
        long_call(p, (combo, "moved to the hooks library"))
        check_pairs(got, X[:, k:], pairs, N - k, every, first, band, exact, (combo, "moved to the hooks library"))
        q.covariance(to_dev(tail), every, first, bins=band)
        check_state(p, q, exact, (combo, "moved to the hooks library"))
        # the pair list moved as well
        p.reset()
        cs = p.cross_sum(to_dev(head), every, first, bins=band)
        assert p.get_option("last_kernel") == 8
        check_pairs(cs, X[:, :k], TILES_PAIRS, k, every, first, band, exact, (combo, "the pair list after the move"))


# ---------------------------------------------------------------------------------------------
# 8. all seven analysis entry points interleaved on a batched plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("m", [125, 1000])
@pytest.mark.parametrize("combo,opts", BOUNDED, ids=case_id)
def test_analysis_entry_points_interleaved_with_covariance(combo, opts, m, seed):
    """test_analysis_entry_points_interleaved_on_a_batched_plan with covariance as the seventh kind: the call reserves a workspace
    of its own, cuts time by block items and writes the state through its own writers, so a call that follows it or that it
    follows is where a stale workspace, a wrong flip of the state buffers or a channel left unwritten shows"""
    run_interleaved(combo, opts, m, seed, channels=4, covariance=True)
