"""The pooled cross-spectrum call (sdft_hip_sdft_cross_sum_n, SDFT.cross_sum) on the routes tests/test_gpu_cross_sum.py leaves to
its siblings' tests, on a real MI355X: forced carry routes on both FD types with the carry form asserted, a state the host
installed, pair lists that exercise the table of writers, device samples with host sums and segments bound by the samples' bytes,
tiles that change under an installed list, and all six analysis entry points interleaved on a batched plan.

References and bars are those of tests/test_gpu_cross_sum.py: the oracle's rows (rows_of), numpy's unfused expression on them
(terms), check_pairs' bar -- gamma_L sum |term| on the bit-identical routes, L BAR max|X_a| max|X_b| on top for FD double's default
carries -- and, where only the library's order of addition defines the bits, the library's own value from a plan that took the
default exact route.  States are compared bit for bit on the exact routes and to 1e-10 of the largest value elsewhere.

The carry form: the relay form needs a block length of 8 ... 128 steps that divides 2 x dftsize.  None divides 250, so a plan of
125 bins takes the serial pass whatever option "chain" says; a plan of 1000 bins takes the relay form (blocks of 8 or 16).  The
cases that are about the form therefore run at 1000 bins as well, and every case asserts the form it ran
(tests/cpp/cross_sum_logic_test.cpp pins the same decisions without a GPU)."""

import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from sdft_amd.sdft import SDFT, power_sum_rows
from sdft_amd.signals import noise
from test_gpu_cross_sum import CH, PAIRS, check_pairs, check_state, plan, rows_of, same_bits, signals, terms
from test_gpu_filterbank import BOUNDED, EXACT, run_interleaved, same_state
from test_gpu_power import exact_combo, make, rel, to_dev

pytestmark = pytest.mark.gpu
N = 6000                                                     # several time chunks, and a roll-over of the cursor at 2 x dftsize
BANDS = {125: (1, 123), 1000: (50, 100)}                     # (the second crosses the first tile boundaries)
DEFAULT_EXACT = dict(EXACT)                                  # combo -> the options of its default exact route
assert DEFAULT_EXACT["f32f32"] == {} and DEFAULT_EXACT["f32f64"] == {"carry": 1} and len(BOUNDED) == 2


def relay_possible(m):
    """a block length of the relay form divides 2 m (logic::relay_block; the chunk lengths of these tests are multiples of 8)"""
    return any((2 * m) % block == 0 for block in (8, 16, 32, 64, 128))


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def assert_route(p, opts, exact, m, what, kernel=8):
    """the route a long call took: forward_cross_sum_kernel (kernel = 9: forward_covariance_kernel) on several chunks, never the
    flow form; the forced chunk and segment count; the relay form (last_chain == 3) wherever the carries are exact, the form is not
    turned off and a block exists, else the serial pass or the partial sums (0)"""
    assert p.get_option("last_kernel") == kernel and p.get_option("last_chunks") > 1 and p.get_option("last_flow") == 0, what
    if "chunk" in opts:
        assert p.get_option("last_chunk_len") == opts["chunk"], what
    if "segments" in opts:
        assert p.get_option("last_segments") == opts["segments"], what
    relay = exact and opts.get("chain", 1) != 0 and relay_possible(m)
    assert p.get_option("last_chain") == (3 if relay else 0), (what, p.get_option("last_chain"))


# ---------------------------------------------------------------------------------------------
# 1. forced routes, both FD types
# ---------------------------------------------------------------------------------------------
ROUTES = {"f32f64": [dict(chunk=128), dict(chunk=1000), dict(carry=1, segments=3), dict(carry=1, chain=2), dict(carry=1, chain=0)],
          "f32f32": [{}, dict(segments=3), dict(chain=2), dict(chain=0), dict(chunk=128)]}
# (one shape after the other: rows_of keeps two)
ROUTE_CASES = [(combo, m, opts) for m in (125, 1000) for combo in ("f32f64", "f32f32") for opts in ROUTES[combo]]


def case_id(v):
    return ("-".join(f"{k}{x}" for k, x in v.items()) or "default") if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("combo,m,opts", ROUTE_CASES, ids=case_id)
def test_cross_sum_forced_routes_both_fd_types(combo, m, opts):
    """the option sets of test_power_sum_forced_routes and test_filterbank_forced_routes on FD double, and the carry forms of FD
    float (exact by default): device samples, three grids.  On the exact routes every value is within gamma_L sum |term|, at
    (1, 0) the expression's bits (check_pairs) and the bits of the default exact route (windows of one sample do not depend on
    where the chunks cut), and the state is the one sdft leaves, bit for bit.  On the serial form side b reads its own channel's
    seed, on the relay form it takes side a's fid: both run here at 1000 bins."""
    band = BANDS[m]
    x, X = rows_of(combo, "hann", m, N)
    dx = to_dev(x)
    exact = exact_combo(combo) or "carry" in opts
    with plan(m, "hann", combo, **opts) as p, make(m, "hann", combo, channels=CH, **opts) as q, plan(m, "hann", combo, **DEFAULT_EXACT[combo]) as d:
        q.sdft(x)
        cache = {}
        for every, first in [(1, 0), (100, 37), (N, 0)]:
            what = (combo, m, opts, every, first)
            p.reset()
            got = p.cross_sum(dx, every, first, bins=band)
            assert_route(p, opts, exact, m, what)
            check_pairs(got, X, PAIRS, N, every, first, band, exact, what, cache=cache)
            check_state(p, q, exact, what)
            if exact and (every, first) == (1, 0):
                d.reset()
                assert same_bits(numpy_of(got), numpy_of(d.cross_sum(dx, every, first, bins=band))), what
                assert_route(d, DEFAULT_EXACT[combo], True, m, (what, "default exact route"))


@pytest.mark.parametrize("every,first", [(1, 0), (100, 37)])
def test_cross_sum_relay_form_from_a_cursor_inside_a_block(every, first):
    """FD float, 1000 bins: a first call of 700 samples leaves the cursor at 700, a multiple of no block length, so the chunks of
    the long call on the next 5300 samples are shifted to begin on block boundaries (chunk j starts at j * len - shift)"""
    combo, m, k = "f32f32", 1000, 700
    band = BANDS[m]
    x, X = rows_of(combo, "hann", m, N)
    with plan(m, "hann", combo) as p, make(m, "hann", combo, channels=CH) as q:
        p.power(np.ascontiguousarray(x[:, :k]), 7, 3, bins=(0, m))
        assert p.get_option("cursor") == k and all(k % block for block in (8, 16, 32, 64, 128))
        got = p.cross_sum(to_dev(x[:, k:]), every, first, bins=band)
        assert_route(p, {}, True, m, (every, first))
        assert p.get_option("last_chain") == 3
        check_pairs(got, X[:, k:], PAIRS, N - k, every, first, band, True, ("from cursor 700", every, first))
        q.sdft(np.ascontiguousarray(x[:, :k])); q.sdft(np.ascontiguousarray(x[:, k:]))
        check_state(p, q, True, ("from cursor 700", every, first))


# ---------------------------------------------------------------------------------------------
# 2. a state installed by the host: the fid no longer counts as canonical, the serial form is taken
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [125, 1000])
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_cross_sum_after_a_state_installed_by_the_host(combo, opts, m):
    """plan p runs sdft over 1500 samples; its state goes to a fresh plan r through sdft_hip_set_state.  Both then make the
    cross-spectrum call on the next 4500 samples: r on the serial form (side b from its own channel's seed), p -- at 1000 bins -- on
    the relay form.  (1, 0): the same bits, the expression's bits; (100, 37): both within the bar; afterwards the same state, all
    four channels, bit for bit, and the one sdft leaves."""
    band, k = BANDS[m], 1500
    x, X = rows_of(combo, "hann", m, N)
    head, tail = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
    for every, first in [(1, 0), (100, 37)]:
        what = (combo, m, every, first)
        with plan(m, "hann", combo, **opts) as p, plan(m, "hann", combo, **opts) as r, make(m, "hann", combo, channels=CH, **opts) as q:
            p.sdft(head); q.sdft(head)
            r.set_state(*p.state())
            assert same_state(p, r), what
            gp = numpy_of(p.cross_sum(to_dev(tail), every, first, bins=band))
            assert_route(p, opts, True, m, (what, "p"))
            gr = numpy_of(r.cross_sum(to_dev(tail), every, first, bins=band))
            assert_route(r, dict(opts, chain=0), True, m, (what, "r"))
            assert r.get_option("last_chain") == 0 and p.get_option("last_chain") == (3 if relay_possible(m) else 0), what
            check_pairs(gp, X[:, k:], PAIRS, N - k, every, first, band, True, (what, "p"))
            check_pairs(gr, X[:, k:], PAIRS, N - k, every, first, band, True, (what, "r"))
            if (every, first) == (1, 0):
                assert same_bits(gp, gr), what
                cols = slice(band[0], band[0] + band[1])
                re, im = terms(X[0][k:, cols], X[2][k:, cols])            # PAIRS[4] = (0, 2): two independent channels
                assert PAIRS[4] == (0, 2) and same_bits(gr[4].real, re) and same_bits(gr[4].imag, im), what
            assert same_state(p, r), what
            q.sdft(tail)
            check_state(p, q, True, what)
            check_state(r, q, True, what)


@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_cross_sum_after_a_state_with_a_fid_of_its_own_per_channel(combo, opts):
    """The channels of a plan share the cursor, so the fids the library itself leaves are the same numbers in every channel, and
    a kernel that read channel a's seed for side b would give the same bits.  Here the host installs a state in which channel c's
    fid is (1 + c / 1024) times the one sdft left (exact in both FD types): the serial form has to hand each side its own channel's
    seed.  The reference is numpy's unfused expression on the rows a twin plan's sdft gives from the same installed state -- at
    (1, 0) bit for bit, at (100, 37) within the bar of an exact route -- and the twin's state afterwards, bit for bit."""
    m, k = 125, 1500
    band = BANDS[m]
    cols = slice(band[0], band[0] + band[1])
    x, X = rows_of(combo, "hann", m, N)
    head, tail = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
    with make(m, "hann", combo, channels=CH, **opts) as t:
        t.sdft(head)
        acc, fid, hist, cursor = t.state()
        fid = fid * (1 + np.arange(CH) / 1024).astype(fid.real.dtype)[:, None]
        assert fid.dtype == X.dtype and not np.array_equal(fid[0], fid[2])
        t.set_state(acc, fid, hist, cursor)
        rows = t.sdft(tail)
        assert t.get_option("last_chain") == 0 and t.get_option("last_chunks") > 1
        assert np.array_equal(rows[0], X[0, k:]) and not np.array_equal(rows[2][:, cols], X[2, k:, cols])     # (the fid matters)
        for every, first in [(1, 0), (100, 37)]:
            what = (combo, "fid per channel", every, first)
            with plan(m, "hann", combo, **opts) as r:
                r.set_state(acc, fid, hist, cursor)
                got = numpy_of(r.cross_sum(to_dev(tail), every, first, bins=band))
                assert_route(r, dict(opts, chain=0), True, m, what)
                if (every, first) == (1, 0):
                    for j, (a, b) in enumerate(PAIRS):
                        re, im = terms(rows[a][:, cols], rows[b][:, cols])
                        assert same_bits(got[j].real, re) and same_bits(got[j].imag, im), (what, (a, b))
                check_pairs(got, rows, PAIRS, N - k, every, first, band, True, what)
                assert same_state(r, t), what


# ---------------------------------------------------------------------------------------------
# 3. pair lists that exercise the table of writers
# ---------------------------------------------------------------------------------------------
def seventy_pairs():
    """70 pairs of 5 channels, drawn: more work items than a workgroup has waves (4), most of them writers of nothing, with
    repeats and both orders of a pair"""
    rng = np.random.default_rng(70)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 5, (70, 2))]
    pairs[10] = pairs[3]
    a, b = next(q for q in pairs if q[0] != q[1])
    pairs[20], pairs[40] = (a, b), (b, a)
    return pairs


WRITER_LISTS = {"a-only": [(0, 1), (2, 1)],                  # item 1 writes side a only, a != b; channels 3 and 4 are advance-only
                "b-only-then-none": [(0, 1), (0, 2), (1, 2)],   # item 1 writes side b only, item 2 writes nothing; 3 and 4 advance-only
                "auto-first": [(4, 4), (0, 4)],              # an auto-pair, then side a only; the unnamed 1, 2, 3 between named channels
                "seventy": seventy_pairs()}
WRITER_ROUTES = [("f32f32", {}), ("f32f64", {"carry": 1}), ("f32f64", {})]


def writers_of(pairs, channels):
    """(writes_a, writes_b) per pair as sdft_hip_set_pairs decides them -- the first item that names a channel writes it, side a
    before side b -- restated here only to assert that the lists are the cases their names claim"""
    written, flags = set(), []
    for a, b in pairs:
        wa = a not in written
        written.add(a)
        wb = b not in written
        written.add(b)
        flags.append((wa, wb))
    return flags, [c for c in range(channels) if c not in written]


def test_writer_lists_are_the_cases_they_claim():
    w = {name: writers_of(pairs, 5) for name, pairs in WRITER_LISTS.items()}
    assert w["a-only"] == ([(True, True), (True, False)], [3, 4])
    assert w["b-only-then-none"] == ([(True, True), (False, True), (False, False)], [3, 4])
    assert w["auto-first"] == ([(True, False), (True, False)], [1, 2, 3])
    flags, unnamed = w["seventy"]
    pairs = WRITER_LISTS["seventy"]
    assert len(pairs) == 70 and unnamed == [] and sum(1 for f in flags if f == (False, False)) >= 60
    assert len(set(pairs)) < len(pairs) and any((b, a) in pairs for a, b in pairs if a != b)


@pytest.mark.parametrize("name", list(WRITER_LISTS))
@pytest.mark.parametrize("combo,opts", WRITER_ROUTES, ids=case_id)
def test_cross_sum_pair_lists_and_their_writers(combo, opts, name):
    """5 channels, 64 bins, 3000 samples.  The values against the oracle's rows; every (b, a) the conjugate of its (a, b) and
    every repeat the same bits; afterwards the state of all five channels is the one sdft leaves on a twin plan -- a channel whose
    writer is side a of an item whose side b writes nothing, side b alone, an advance-only item between named channels -- and a
    following sdft of 100 samples gives the twin's rows.  Bit for bit on the exact routes, 1e-10 with FD double's default carries."""
    pairs = WRITER_LISTS[name]
    ch, m, n = 5, 64, 3000
    td = O.combo_types(combo)[0]
    exact = exact_combo(combo) or "carry" in opts
    x, X = rows_of(combo, "hann", m, n, None, ch)
    assert np.array_equal(x, signals(td, n, m, ch)) and np.array_equal(x[1], x[0] * td(0.5)) and not np.array_equal(x[3], x[4])
    hop = np.stack([noise(100, seed=12 + c, dtype=td) for c in range(ch)])
    with plan(m, "hann", combo, pairs=pairs, channels=ch, **opts) as p, make(m, "hann", combo, channels=ch, **opts) as q:
        tiles, per = p.get_option("tiles"), p.get_option("interior") * p.get_option("bins_per_lane")
        band = (per - 2, 4) if tiles > 1 else (1, m - 2)      # across the first tile boundary where the plan has one
        assert band[0] + band[1] <= m and (tiles == 1 or band[0] < per < band[0] + band[1])
        cache = {}
        for i, (every, first) in enumerate([(1, 0), (7, 3)]):
            what = (combo, opts, name, every, first)
            p.reset(); q.reset()
            s = numpy_of(p.cross_sum(to_dev(x) if i else x, every, first, bins=band))
            assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1, what
            check_pairs(s, X, pairs, n, every, first, band, exact, what, cache=cache)
            place = {}
            for j, (a, b) in enumerate(pairs):
                if (a, b) in place:
                    assert same_bits(s[j], s[place[(a, b)]]), (what, "repeat", j, (a, b))
                if a != b and (b, a) in place:
                    ba = s[place[(b, a)]]
                    assert same_bits(s[j].real, ba.real) and np.array_equal(s[j].imag, -ba.imag), (what, "conjugate", j, (a, b))
                if a == b:
                    assert same_bits(s[j].imag, np.zeros_like(s[j].imag)), (what, "auto-pair", j)
                place.setdefault((a, b), j)
            q.sdft(x)
            check_state(p, q, exact, what)
            dp, dq = p.sdft(hop), q.sdft(hop)
            if exact:
                assert same_bits(dp, dq), what
            else:
                assert rel(dp, dq) <= 1e-10, (what, rel(dp, dq))
            check_state(p, q, exact, (what, "after the hop"))


# ---------------------------------------------------------------------------------------------
# 4. device samples with host sums; segments bound by the samples' bytes
# ---------------------------------------------------------------------------------------------
def raw_cross_sum(p, x, n, every, first, band, sums):
    ptr = lambda a: C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    p.api.clear()
    got = p.api.sdft_cross_sum_n(p._p, n, ptr(x), every, first, band[0], band[1], ptr(sums))
    p.synchronize()
    assert got == power_sum_rows(n, every, first), (got, p.api.last_error())
    assert p.get_option("last_kernel") == 8


def sentinel_sums(fd, rows, nb, device, npairs=len(PAIRS)):
    """sums no call has written: NaN in every number (a head row added to an unwritten row stays NaN, too)"""
    import torch
    cd = np.complex64 if fd == np.float32 else np.complex128
    if device:
        return torch.full((npairs, rows, nb), complex(float("nan"), float("nan")), dtype=getattr(torch, np.dtype(cd).name), device="cuda")
    return np.full((npairs, rows, nb), complex(np.nan, np.nan), dtype=cd)


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_cross_sum_staging_device_samples_host_sums_and_sample_bound_segments(combo):
    """stage_bytes of 7 and of 2 rows of sums with device samples and host sums (per-pair copies through device scratch, head
    rows added on the host): windows shorter than a segment, longer than one, one window over all segments, heads that join
    (first % every != 0) and segments of whole windows; stage_bytes of 700 samples with host samples, where the samples' bytes
    bound the segment, into host and into device sums (there (6000, 0) is one window over nine segments, every later one a head the
    host adds).  Every element is written, the values are within the contract's bar, on
    FD float at (1, 0) they are the bits of the unstaged device-to-device call, and the state is that call's."""
    td, fd, _ = O.combo_types(combo)
    m, band = 125, (10, 100)
    exact = exact_combo(combo)
    x, X = rows_of(combo, "hann", m, N)
    dx = to_dev(x)
    row = len(PAIRS) * 2 * band[1] * np.dtype(fd).itemsize
    one = [(1, 0)] if exact else []
    runs = [("device samples, host sums", 7 * row, dx, False, [(100, 37), (100, 0)] + one),
            ("device samples, host sums", 2 * row, dx, False, [(1024, 1023), (N, 0), (700, 0)]),
            ("host samples, host sums", 700 * CH * np.dtype(td).itemsize, x, False, [(100, 37), (700, 699), (N, 0)]),
            ("host samples, device sums", 700 * CH * np.dtype(td).itemsize, x, True, [(100, 37), (700, 699)] + one)]
    with plan(m, "hann", combo) as q:
        for kind, stage, xs, device_sums, grids in runs:
            with plan(m, "hann", combo, stage_bytes=stage) as p:
                for every, first in grids:
                    what = (combo, kind, stage, every, first)
                    rows = power_sum_rows(N, every, first)
                    q.reset()
                    want = numpy_of(q.cross_sum(dx, every, first, bins=band))
                    p.reset()
                    out = sentinel_sums(fd, rows, band[1], device_sums)
                    raw_cross_sum(p, xs, N, every, first, band, out)
                    out = numpy_of(out)
                    assert out.shape == want.shape and not np.isnan(out.real).any() and not np.isnan(out.imag).any(), (what, "a sum was left unwritten")
                    check_pairs(out, X, PAIRS, N, every, first, band, exact, what)
                    if exact and (every, first) == (1, 0):
                        assert same_bits(out, want), what
                    assert same_state(p, q) if exact else p.state()[3] == q.state()[3], what


# ---------------------------------------------------------------------------------------------
# 5. option "interior" changes the tiles under an installed pair list
# ---------------------------------------------------------------------------------------------
def hooked(combo, opts, hooks=True):
    p = SDFT(1024, "hann", 1.0, combo, channels=CH, hooks=hooks)
    for k, v in opts.items():
        p.set_option(k, v)
    p.set_pairs([a for a, _ in PAIRS], [b for _, b in PAIRS])
    return p


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {})])
def test_cross_sum_when_the_tiles_change_under_an_installed_list(combo, opts):
    """the counterpart of test_filterbank_is_cut_again_when_the_tiles_change: the workspace of the cut windows and the tiles' test
    against the band follow the tiles of the call, the list stays installed; and a list installed in the product library moves
    with the plan to the hooks library (SDFT.set_option replays it) together with the state"""
    m, every, first, band, other = 1024, 7, 6, (50, 100), 62
    exact = exact_combo(combo) or "carry" in opts
    x, X = rows_of(combo, "hann", m, N)
    with hooked(combo, opts) as p:
        assert p.get_option("test_hooks") == 1
        tiles0, interior0 = p.get_option("tiles"), p.get_option("interior")
        assert interior0 != other
        outs, cache = [], {}
        for step, lanes in enumerate((interior0, other, interior0)):
            p.set_option("interior", lanes)
            assert p.get_option("interior") == lanes and (p.get_option("tiles") != tiles0) == (lanes != interior0)
            p.reset()
            outs.append(numpy_of(p.cross_sum(to_dev(x) if step % 2 else x, every, first, bins=band)))
            assert p.pairs == len(PAIRS) and p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
            check_pairs(outs[-1], X, PAIRS, N, every, first, band, exact, (combo, "interior", lanes), cache=cache)
        assert same_bits(outs[0], outs[2]), combo
    # installed in the product library, a call, then an option only the hooks library knows
    k = 700
    head, tail = np.ascontiguousarray(x[:, :k]), np.ascontiguousarray(x[:, k:])
    with hooked(combo, opts, hooks=False) as p, hooked(combo, opts, hooks=False) as q:
        assert p.get_option("test_hooks") == 0
        first_part = p.cross_sum(head, every, first, bins=band)
        assert same_bits(first_part, q.cross_sum(head, every, first, bins=band))
        p.set_option("interior", other)
        assert p.get_option("test_hooks") == 1 and p.get_option("interior") == other and p.get_option("tiles") != tiles0
        assert q.get_option("test_hooks") == 0 and q.get_option("tiles") == tiles0
        assert p.pairs == len(PAIRS)
        assert p.state()[3] == k and (same_state(p, q) if exact else p.state()[3] == q.state()[3])
        got = numpy_of(p.cross_sum(to_dev(tail), every, first, bins=band))
        assert p.get_option("last_kernel") == 8 and p.get_option("last_chunks") > 1
        check_pairs(got, X[:, k:], PAIRS, N - k, every, first, band, exact, (combo, "moved to the hooks library"))
        q.cross_sum(to_dev(tail), every, first, bins=band)
        check_state(p, q, exact, (combo, "moved to the hooks library"))


# ---------------------------------------------------------------------------------------------
# 6. all six analysis entry points interleaved on a batched plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("m", [125, 1000])
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_analysis_entry_points_interleaved_on_a_batched_plan(combo, opts, m, seed):
    """test_analysis_entry_points_interleaved_on_one_plan (tests/test_gpu_filterbank.py, run_interleaved) on a plan of 4 channels
    with cross_sum as the sixth kind: the call launches by work items, so it cuts time differently from its siblings, reserves a
    workspace of its own and writes the state through its table of writers; a call that follows it or that it follows is where a
    stale workspace, a wrong flip of the state buffers or a channel left unwritten shows"""
    run_interleaved(combo, opts, m, seed, channels=CH)
