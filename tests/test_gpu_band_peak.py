"""Band-peak analysis (sdft_hip_sdft_band_peak_n, SDFT.band_peak) on a real MI355X.

Every comparison is bitwise: the value viewed as integers (NaN equal to NaN), the bin equal.  The expected pair of a row and a band
is the header's numpy expression: with v = w * p in the FD dtype (one rounded product per bin) over the band's bins in ascending
order, i = np.argmax(v) and m = v[i].  p is the oracle's power on the routes where sdft_sdft_n is bit-identical to the reference (FD
float, FD double with option carry = 1, calls shorter than 512 samples) and a twin plan's power() elsewhere, so no route needs a
tolerance.  Large cases evaluate the same expression on the device (peaks_on_device: the largest value by amax, the lowest bin that
holds it by a min over indices -- no argmax whose tie rule would have to be trusted); test_device_expression_is_numpy_argmax holds
that evaluation against np.argmax on vectors full of ties, zeros of both signs, inf and NaN."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd import filterbank as F
from test_gpu_power import ROOT, WINDOWS, exact_combo, expected, make, power_of, signal, to_dev
from test_gpu_filterbank import (BOUNDED, EXACT, FB_BOUND, GRIDS, four_tile_plan, geometry, host_link, in_fd, one_bin_bands, pieces_of,
                                 random_bands, same_state, slots_of, split_bank, whole_row)

pytestmark = pytest.mark.gpu
MS = (1, 2, 3, 5, 64, 125, 1000)


def exact_opts(combo):
    """the options that put a type pair on a route bit-identical to the reference"""
    return {} if exact_combo(combo) else {"carry": 1}


def banks_of(m):
    banks = [("whole row", whole_row(m)), ("one-bin bands", one_bin_bands(m)), ("random", random_bands(m))]
    if m >= 64:
        banks.append(("mel", F.mel(m, 48000, min(40, m))))
    return banks


# ---------------------------------------------------------------------------------------------
# the expected pairs
# ---------------------------------------------------------------------------------------------
def peaks_numpy(bank, p):
    """[rows][nbands][2] from the powers p [rows][m] (FD dtype), the weights in the FD dtype: np.argmax / take on fl(w * p)"""
    b0, nb, w = (np.asarray(a) for a in bank)
    assert w.dtype == p.dtype
    out = np.empty((p.shape[0], b0.size, 2), dtype=p.dtype)
    rows = np.arange(p.shape[0])
    off = 0
    for b in range(b0.size):
        s, k = int(b0[b]), int(nb[b])
        v = w[off:off + k] * p[:, s:s + k]
        i = np.argmax(v, axis=1) if p.shape[0] else np.zeros(0, dtype=np.int64)
        out[:, b, 0] = v[rows, i]
        out[:, b, 1] = s + i
        off += k
    return out


def peaks_on_device(bank, p):
    """the same pairs, evaluated on the device from a device tensor p: the value is NaN if the band holds one, else the largest v;
    the bin is the lowest one that holds a NaN, else the lowest one equal to the largest (zeros of either sign are equal)"""
    import torch
    b0, nb, w = (np.asarray(a) for a in bank)
    wd = torch.from_numpy(w).cuda()
    assert wd.dtype == p.dtype
    out = torch.empty((p.shape[0], b0.size, 2), dtype=p.dtype, device="cuda")
    off = 0
    for b in range(b0.size):
        s, k = int(b0[b]), int(nb[b])
        v = wd[off:off + k] * p[:, s:s + k]
        nan = torch.isnan(v)
        top = torch.where(nan, torch.full_like(v, -np.inf), v).amax(dim=1, keepdim=True)
        hit = torch.where(nan.any(dim=1, keepdim=True), nan, v == top)
        at = torch.where(hit, torch.arange(k, device="cuda"), k).amin(dim=1)
        out[:, b, 0] = v.gather(1, at[:, None])[:, 0]
        out[:, b, 1] = (at + s).to(p.dtype)
        off += k
    return out


def peaks_of(bank, p):
    """numpy where it is quick, the device elsewhere; p numpy, the result a numpy array or a device tensor"""
    work = p.shape[0] * int(np.asarray(bank[1]).sum())
    return peaks_numpy(bank, np.asarray(p)) if work <= 3e7 else peaks_on_device(bank, to_dev(p))


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_pairs(got, want, nan_payload=False):
    """shape, dtype, the values' bits and the bins; nan_payload: a NaN equals any NaN (its payload is unspecified)"""
    import torch
    if (hasattr(got, "cpu") or hasattr(want, "cpu")) and not nan_payload:          # (on the device: these arrays reach gigabytes)
        got, want = (v if hasattr(v, "cpu") else torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (got, want))
        iv = torch.int32 if got.dtype == torch.float32 else torch.int64
        return got.shape == want.shape and got.dtype == want.dtype and bool(torch.equal(got.contiguous().view(iv), want.contiguous().view(iv)))
    g, w = (np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (got, want))
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if not nan_payload:
        return g.tobytes() == w.tobytes()
    both = np.isnan(g[..., 0]) & np.isnan(w[..., 0])
    return bool(((bits(g[..., 0]) == bits(w[..., 0])) | both).all()) and np.array_equal(g[..., 1], w[..., 1])


def test_device_expression_is_numpy_argmax():
    rng = np.random.default_rng(3)
    for fd in (np.float32, np.float64):
        alphabet = np.array([0.0, -0.0, 1.0, 1.0, -0.5, -2.0, np.inf, -np.inf, np.nan, 2.0 ** -140], dtype=fd)
        p = alphabet[rng.integers(0, alphabet.size, (3000, 40))]
        p[:1000] = alphabet[:6][rng.integers(0, 6, (1000, 40))]
        p[1000:1500] = alphabet[:2][rng.integers(0, 2, (500, 40))]
        bank = in_fd(random_bands(40, seed=5), fd)
        want, got = peaks_numpy(bank, p), peaks_on_device(bank, to_dev(p))
        assert same_pairs(got, want, nan_payload=True)
        assert np.isnan(want[..., 0]).any() and (want[..., 0] == 0).any() and np.signbit(want[..., 0][want[..., 0] == 0]).any()


# ---------------------------------------------------------------------------------------------
# (1) parity on the exact routes
# ---------------------------------------------------------------------------------------------
def run_parity(m, n, window, combo):
    fd = O.combo_types(combo)[1]
    x, pw = expected(combo, window, m, n)
    dx = to_dev(x)
    with make(m, window, combo, **exact_opts(combo)) as p:
        for b, (name, bank) in enumerate(banks_of(m)):
            bank = in_fd(bank, fd)
            p.set_filterbank(*bank)
            want = peaks_of(bank, pw)
            for g, (every, first) in enumerate(GRIDS):
                p.reset()
                got = p.band_peak(dx if (b + g) % 2 else x, every, first)          # host and device memory alternate
                what = (combo, window, m, name, every, first)
                assert p.get_option("last_kernel") == 14, what
                if m >= 1000:
                    assert p.get_option("last_chunks") > 1, what
                assert tuple(got.shape) == (len(range(first, n, every)), bank[0].size, 2), what
                assert same_pairs(got, want[first::every]), what
                del got
            del want


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("m", MS)
def test_band_peak_parity(m, window, combo):
    run_parity(m, 6000, window, combo)                       # several chunks, and a roll-over at 2N


@pytest.mark.parametrize("combo", O.COMBOS)
def test_band_peak_parity_more_than_one_bin_per_lane(combo):
    run_parity(4096, 10000, "hann", combo)


# ---------------------------------------------------------------------------------------------
# (2) ties across a tile boundary
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT)
def test_band_peak_ties_across_a_tile_boundary(combo, opts):
    """The plan's own tiles, then tiles of 62 lanes (the hooks library's option): the bands (60, 4), (61, 2) and (61, 63), which
    straddle the boundaries of tiles of 62 bins, and bands across the geometry's own first boundaries.  All-zero weights on a live
    signal, then weight 1 on a silent one: every value is a zero and the bin is the band's first, which lies in the lower tile.
    One band has a single non-zero weight, on its last bin, in its last tile."""
    from sdft_amd.sdft import SDFT
    td, fd, _ = O.combo_types(combo)
    m, n = 1000, 700
    x = signal(n, td, 3)
    with make(m, "hann", combo, **opts) as q:
        pw = q.power(x)
    with SDFT(m, "hann", 1.0, combo, hooks=True) as p:
        for k, v in opts.items():
            p.set_option(k, v)
        for lanes in (p.get_option("interior"), 62):
            p.set_option("interior", lanes)
            tiles, per = geometry(p)
            assert tiles >= 3
            lone = (per - 1, per + 2)                        # bins per - 1 ... 2 per: three tiles, the weight on bin 2 per
            bands = [(60, 4), (61, 2), (61, 63), (per - 2, 4), (per - 1, 2), lone, (0, m)]
            b0 = np.array([s for s, _ in bands], dtype=np.uint64)
            nb = np.array([k for _, k in bands], dtype=np.uint64)
            assert (pieces_of((b0, nb), per)[3:] > 1).all() and pieces_of((b0, nb), per)[5] == 3
            if lanes == 62 and per == 62:
                assert (pieces_of((b0, nb), per)[:3] > 1).all()
            total = int(nb.sum())
            for case, (w, xs) in enumerate([(np.zeros(total), x), (np.ones(total), np.zeros(n, dtype=td))]):
                w = w.astype(fd)
                if case == 0:
                    w[int(nb[:5].sum()) + lone[1] - 1] = 0.75
                p.set_filterbank(b0, nb, w)
                p.reset()
                got = p.band_peak(to_dev(xs) if case else xs, 1, 0)
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                assert p.get_option("last_kernel") == 14
                for j, (s, k) in enumerate(bands):
                    if case == 0 and j == 5:
                        last = s + k - 1
                        want = fd(0.75) * pw[:, last]
                        assert last // per == 2 and (want > 0).all()
                        assert np.array_equal(bits(got[:, j, 0]), bits(want)) and (got[:, j, 1] == last).all(), (combo, lanes, case, s, k)
                        continue
                    assert (bits(got[:, j, 0]) == 0).all(), (combo, lanes, case, s, k)      # +0: the first bin's bits
                    assert (got[:, j, 1] == s).all(), (combo, lanes, case, s, k, np.unique(got[:, j, 1]))


# ---------------------------------------------------------------------------------------------
# (3) one-bin bands of weight 1 are the power call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_one_bin_bands_are_the_power_call_and_bin_k(combo):
    """one chunk; chunk-parallel (default FD double: the inexact route, against a twin with the same chunk); exact carries; host
    and device memory"""
    td, fd, _ = O.combo_types(combo)
    call = 0
    for m, n, opts in ((64, 500, {}), (125, 6000, {}), (1000, 6000, {}), (1024, 6000, {"carry": 1})):
        x = signal(n, td, m)
        with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
            p.set_filterbank(*in_fd(one_bin_bands(m), fd))
            for every, first in GRIDS[:3]:
                p.reset(); q.reset()
                call += 1
                xs = to_dev(x) if call % 2 else x
                got, want = p.band_peak(xs, every, first), q.power(xs, every, first)
                assert p.get_option("last_kernel") == 14 and q.get_option("last_kernel") == 5
                assert (p.get_option("last_chunks"), p.get_option("last_chunk_len")) == (q.get_option("last_chunks"), q.get_option("last_chunk_len"))
                got, want = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (got, want))
                assert got.shape == want.shape + (2,) and got.dtype == want.dtype
                assert np.array_equal(bits(got[..., 0]), bits(want)), (combo, m, every, first)
                assert np.array_equal(got[..., 1], np.broadcast_to(np.arange(m, dtype=fd), want.shape)), (combo, m, every, first)


# ---------------------------------------------------------------------------------------------
# (4) the inexact route: the expression on a twin plan's powers; determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_band_peak_inexact_route_is_the_expression_on_the_twins_powers(combo):
    td, fd, _ = O.combo_types(combo)
    m, n = 1000, 6000
    x = signal(n, td, 77)
    bank = in_fd(random_bands(m), fd)
    outs = []
    for _ in range(2):
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            p.set_filterbank(*bank)
            got = p.band_peak(to_dev(x), 1, 0)
            pw = q.power(to_dev(x), 1, 0)
            assert p.get_option("last_kernel") == 14 and p.get_option("last_chunks") > 1
            assert p.get_option("last_chunk_len") == q.get_option("last_chunk_len") and p.get_option("last_chunks") == q.get_option("last_chunks")
            assert same_pairs(got, peaks_on_device(bank, pw)), combo
            outs.append(got.cpu().numpy().tobytes())
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------
# (5) streaming and chunking, (6) state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT)
def test_band_peak_streaming_and_chunking_bit_identical(combo, opts):
    from sdft_amd.sdft import every_next_first
    td, fd, _ = O.combo_types(combo)
    m, n = 1000, 6000
    lengths = [1, 511, 512, 513, 3000]
    lengths.append(n - sum(lengths))
    x = signal(n, td, 21)
    bank = in_fd(random_bands(m), fd)
    for every in (1, 100):
        with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
            p.set_filterbank(*bank); q.set_filterbank(*bank)
            whole = p.band_peak(to_dev(x), every, 0).cpu().numpy()
            chunks = p.get_option("last_chunks")
            assert chunks > 1
            got, t, first = [], 0, 0
            for i, k in enumerate(lengths):
                xs = x[t:t + k]
                d = q.band_peak(to_dev(xs) if i % 2 else xs, every, first)
                got.append(d.cpu().numpy() if hasattr(d, "cpu") else d)
                first = every_next_first(k, every, first)
                t += k
            assert same_pairs(np.concatenate(got), whole), (combo, every)
            assert same_state(p, q), (combo, every)
            for forced in (256, 1024):
                p.reset()
                p.set_option("chunk", forced)
                again = p.band_peak(to_dev(x), every, 0).cpu().numpy()
                assert p.get_option("last_chunks") not in (1, chunks), (forced, chunks)
                assert same_pairs(again, whole), (combo, every, forced)
            p.set_option("chunk", 0)


@pytest.mark.parametrize("combo,opts", EXACT)
def test_state_after_a_band_peak_call_is_sdft_n_s(combo, opts):
    td, fd, _ = O.combo_types(combo)
    m, n, more = 1000, 6000, 700
    x = signal(n + more, td, 31)
    with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
        p.set_filterbank(*in_fd(F.mel(m, 48000, 40), fd))
        p.band_peak(to_dev(x[:n]), 100, 5)
        q.sdft(to_dev(x[:n]))
        assert same_state(p, q)
        a, b = p.sdft(x[n:]), q.sdft(x[n:])
        assert np.array_equal(bits(a.view(fd)), bits(b.view(fd))), combo
        assert same_state(p, q)


# ---------------------------------------------------------------------------------------------
# (7) batched plans
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_band_peak_batched_channels(combo, opts):
    td, fd, _ = O.combo_types(combo)
    ch, m, n = 3, 256, 6000
    x = np.stack([signal(n, td, 200 + c) for c in range(ch)])
    bank = in_fd(random_bands(m), fd)
    for device in (False, True):
        for every, first in ((100, 50), (3, 1)):
            with make(m, "blackman", combo, channels=ch, **opts) as p:
                p.set_filterbank(*bank)
                got = p.band_peak(to_dev(x) if device else x, every, first)
                got = got.cpu().numpy() if device else got
                assert p.get_option("last_kernel") == 14
            assert got.shape == (ch, len(range(first, n, every)), bank[0].size, 2)
            for c in range(ch):
                with make(m, "blackman", combo, **opts) as q:
                    q.set_filterbank(*bank)
                    assert same_pairs(got[c], q.band_peak(x[c], every, first)), (combo, device, every, c)


# ---------------------------------------------------------------------------------------------
# (8) beyond the workspace bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every,first", [(1, 0), (3, 2)])
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_band_peak_beyond_the_workspace_bound(combo, opts, every, first):
    """the shape of the filterbank suite's run_beyond_the_bound with a slot of 2 * sizeof(FD): pieces of at least 3 x 64 MiB in one
    device call, against the expression on the oracle's powers, and rows and state against a twin fed in calls of one launch each"""
    import torch
    from sdft_amd.sdft import every_next_first, every_rows
    td, fd, _ = O.combo_types(combo)
    n = 6000
    slot = 2 * np.dtype(fd).itemsize
    rows = every_rows(n, every, first)
    with four_tile_plan(combo, **opts) as p, four_tile_plan(combo, **opts) as q:
        m = p.dftsize
        tiles, per = geometry(p)
        bank = in_fd(split_bank(m, tiles, per, -(-3 * FB_BOUND // (rows * slot))), fd)
        nslots = slots_of(bank, per)
        assert rows * nslots * slot >= 3 * FB_BOUND
        x, pw = expected(combo, "hann", m, n)
        p.set_filterbank(*bank); q.set_filterbank(*bank)
        got = p.band_peak(to_dev(x), every, first)
        launches, chunks = p.get_option("last_band_peak_launches"), p.get_option("last_chunks")
        print(f"{(combo, m, n, every, first)}: {bank[0].size} bands, {nslots} slots, {chunks} chunks in {launches} launches")
        assert p.get_option("last_kernel") == 14
        assert launches >= -(-(rows * nslots * slot) // FB_BOUND)
        assert 3 <= launches < chunks                        # several chunks to a launch, and the last launch ragged
        assert same_pairs(got, peaks_on_device(bank, to_dev(np.ascontiguousarray(pw[first::every])))), (combo, every, first)
        fit = FB_BOUND // (nslots * slot)                    # rows of one launch
        lengths = [1, 511, 512, 513]
        while sum(lengths) < n:
            lengths.append(min(fit * every - 5, n - sum(lengths)))
        parts, t, f = [], 0, first
        for k in lengths:
            parts.append(q.band_peak(to_dev(x[t:t + k]), every, f))
            assert q.get_option("last_band_peak_launches") == 1, (k, f)
            f = every_next_first(k, every, f)
            t += k
        assert same_pairs(torch.cat(parts), got), (combo, every, first)
        assert same_state(p, q), (combo, every, first)


# ---------------------------------------------------------------------------------------------
# (9) host staging
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_band_peak_host_staging_in_segments(combo, opts):
    """stage_bytes of 7 and of 2 output rows: host samples into host and into device output, the rows of the unstaged call bit for bit"""
    import torch
    from sdft_amd.sdft import every_rows
    td, fd, _ = O.combo_types(combo)
    m, n = 1000, 6000
    x = signal(n, td, 61)
    bank = in_fd(random_bands(m), fd)
    nbands = bank[0].size
    row = 2 * nbands * np.dtype(fd).itemsize
    with make(m, "hann", combo, **opts) as q:
        q.set_filterbank(*bank)
        for stage, grids in [(7 * row, [(100, 37), (100, 0), (100, 99)]), (2 * row, [(1024, 1023), (6000, 0), (700, 0)])]:
            with make(m, "hann", combo, stage_bytes=stage, **opts) as p:
                p.set_filterbank(*bank)
                for every, first in grids:
                    rows = every_rows(n, every, first)
                    q.reset()
                    want = q.band_peak(to_dev(x), every, first)
                    p.reset()
                    got = p.band_peak(x, every, first)
                    assert p.get_option("last_kernel") == 14
                    assert same_pairs(got, want.cpu().numpy()), (combo, stage // row, every, first, "host")
                    assert same_state(p, q)
                    p.reset()
                    out = torch.zeros((rows, nbands, 2), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
                    ret = p.api.sdft_band_peak_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, C.c_void_p(out.data_ptr()))
                    p.synchronize()
                    assert ret == rows, p.api.last_error()
                    assert same_pairs(out, want), (combo, stage // row, every, first, "device rows")


# ---------------------------------------------------------------------------------------------
# (10) guarded, misaligned output
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_band_peak_guarded_misaligned_output(combo, opts, host):
    """peaks carved from a guarded arena at residue sizeof(fd) of a 16-byte address -- no pair is aligned to a pair --, an odd
    number of bands, split bands among them"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first = 1000, 2000, 3, 1
    x, pw = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    bank = (bank[0][:-1], bank[1][:-1], bank[2][:int(bank[1][:-1].sum())])
    nbands = bank[0].size
    assert nbands % 2 == 1
    rows = len(range(first, n, every))
    size = np.dtype(fd).itemsize
    with make(m, "hann", combo, **opts) as p:
        tiles, per = geometry(p)
        assert (pieces_of(bank, per) > 1).any()
        p.set_filterbank(*bank)
        arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, nbands, 2), fd)))
        xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
        out = arena.carve((rows, nbands, 2), fd, size, 16, name="peaks")
        assert G.ptr_of(out) % 16 == size
        p.api.clear()
        got = p.api.sdft_band_peak_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, C.c_void_p(G.ptr_of(out)))
        p.synchronize()
        assert got == rows, p.api.last_error()
        assert p.get_option("last_kernel") == 14 and p.get_option("last_chunks") > 1
        arena.check()
        assert G.view_unwritten(out) == 0
        assert np.array_equal(G.to_numpy(xv), x)
        assert same_pairs(np.ascontiguousarray(G.to_numpy(out)), peaks_on_device(bank, to_dev(np.ascontiguousarray(pw[first::every])))), (combo, host)


# ---------------------------------------------------------------------------------------------
# (11) the NaN rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_band_peak_nan_rule(combo):
    """m = 64, n = 400 (one chunk), one NaN sample: the rows before it are the clean run's; from it on every value is NaN and the
    bin the band's first; the expected values come from the twin plan's power()"""
    td, fd, _ = O.combo_types(combo)
    m, n, at = 64, 400, 150
    clean = signal(n, td, 9)
    x = clean.copy()
    x[at] = np.nan
    bank = in_fd(random_bands(m), fd)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        p.set_filterbank(*bank)
        want_clean = p.band_peak(clean)
        assert p.get_option("last_chunks") == 1
        p.reset()
        for device in (False, True):
            p.reset(); q.reset()
            got = p.band_peak(to_dev(x) if device else x)
            got = got.cpu().numpy() if device else got
            pw = q.power(x)
            assert p.get_option("last_kernel") == 14 and p.get_option("last_chunks") == 1
            assert np.isnan(pw[at:]).all() and not np.isnan(pw[:at]).any()
            assert same_pairs(got[:at], want_clean[:at]), combo
            assert np.isnan(got[at:, :, 0]).all(), combo
            assert np.array_equal(got[at:, :, 1], np.broadcast_to(bank[0].astype(fd), (n - at, bank[0].size))), combo
            assert same_pairs(got, peaks_numpy(bank, pw), nan_payload=True), combo


# ---------------------------------------------------------------------------------------------
# (12) the tiles change after the bank was installed
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_band_peak_is_cut_again_when_the_tiles_change(combo, opts):
    from sdft_amd.sdft import SDFT
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, other = 1024, 6000, 7, 6, 62
    x, pw = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    want = peaks_on_device(bank, to_dev(np.ascontiguousarray(pw[first::every])))
    with SDFT(m, "hann", 1.0, combo, hooks=True) as p:
        for k, v in opts.items():
            p.set_option(k, v)
        assert p.get_option("test_hooks") == 1
        p.set_filterbank(*bank)
        tiles0, interior0 = p.get_option("tiles"), p.get_option("interior")
        for step, lanes in enumerate((interior0, other, interior0)):
            p.set_option("interior", lanes)
            assert p.get_option("interior") == lanes and (p.get_option("tiles") != tiles0) == (lanes != interior0)
            p.reset()
            got = p.band_peak(to_dev(x) if step % 2 else x, every, first)
            assert p.get_option("last_kernel") == 14 and p.get_option("last_chunks") > 1
            assert p.filterbank_bands == bank[0].size
            assert same_pairs(got, want), (combo, "interior", lanes)


# ---------------------------------------------------------------------------------------------
# (13) the entry points interleaved on one plan
# ---------------------------------------------------------------------------------------------
def filterbank_numpy(bank, p, per):
    """the filterbank call's value from powers: a band's rounded products added in ascending order inside a tile, then the tiles'
    sums in ascending order (np.cumsum adds one element after the other)"""
    b0, nb, w = (np.asarray(a) for a in bank)
    out = np.empty((p.shape[0], b0.size), dtype=p.dtype)
    off = 0
    for b in range(b0.size):
        s, k = int(b0[b]), int(nb[b])
        v = w[off:off + k] * p[:, s:s + k]
        cuts = [s] + [t for t in range((s // per + 1) * per, s + k, per)] + [s + k]
        sums = np.stack([np.cumsum(v[:, a - s:e - s], axis=1)[:, -1] for a, e in zip(cuts[:-1], cuts[1:])], axis=1)
        out[:, b] = np.cumsum(sums, axis=1)[:, -1]
        off += k
    return out


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_band_peak_interleaved_with_the_other_entry_points(combo, opts, seed):
    """12 000 samples in 25 to 40 calls drawn among sdft, power, filterbank and band_peak on one plan, host and device memory in
    turn; a twin plan takes the same cuts through sdft alone and every output is what numpy derives from its rows of that call"""
    td, fd, _ = O.combo_types(combo)
    m, n = 250, 12000
    rng = np.random.default_rng(1000 + seed)
    special = [1, 2, 99, 100, 511, 512, 513, 2 * m - 1, 2 * m, 2 * m + 1]
    calls = int(rng.integers(25, 41))
    cuts = np.sort(rng.choice(np.arange(1, n - sum(special)), calls - len(special) - 1, replace=False))
    drawn = np.diff(np.concatenate([[0], cuts, [n - sum(special)]]))
    lengths = rng.permutation(np.concatenate([special, drawn]).astype(np.int64))
    assert lengths.size == calls and lengths.sum() == n and (lengths >= 1).all()
    x = signal(n, td, 50 + seed)
    bank = in_fd(random_bands(m), fd)
    names = ("sdft", "power", "filterbank", "band_peak")
    order = rng.permutation(np.resize(np.arange(len(names)), calls))
    with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as twin:
        per = geometry(p)[1]
        assert (pieces_of(bank, per) > 1).any()
        p.set_filterbank(*bank)
        t = 0
        for i, k in enumerate(lengths.tolist()):
            kind = names[int(order[i])]
            every = int(rng.choice([1, 2, 3, 7, 100, int(rng.integers(1, 600))]))
            first = int(rng.integers(0, every + 2))
            xs = np.ascontiguousarray(x[t:t + k])
            xin = to_dev(xs) if i % 2 else xs
            what = (combo, seed, i, kind, k, every, first)
            rows = twin.sdft(xs)
            pw = np.ascontiguousarray(power_of(rows)[first::every])
            if kind == "sdft":
                got, want = p.sdft(xin), rows
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                assert np.array_equal(bits(got.view(fd)), bits(want.view(fd))), what
            elif kind == "power":
                got = p.power(xin, every, first)
                assert np.array_equal(bits(got), bits(pw)), what
            elif kind == "filterbank":
                got = p.filterbank(xin, every, first)
                assert np.array_equal(bits(got), bits(filterbank_numpy(bank, pw, per))), what
            else:
                got = p.band_peak(xin, every, first)
                assert p.get_option("last_kernel") == 14, what
                assert same_pairs(got, peaks_numpy(bank, pw)), what
            assert same_state(p, twin), what
            t += k


# ---------------------------------------------------------------------------------------------
# (14) errors
# The refusal of dftsize > 2^24 on an FD float plan is not run here: a plan of that size is no test of a few seconds (its tables
# and state alone are gigabytes).  What decides it, logic::band_peak_bins_exact, is held in tests/cpp/band_peak_logic_test.cpp; the
# entry point hands its message to grid_args as that call's own refusal, after the grid's checks and before the output's.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_band_peak_out_argument(combo):
    """SDFT.band_peak(out=...): a contiguous array of the samples' kind is written in place and returned; a non-contiguous one of
    the right shape is refused with ValueError and left as it was (a reshape of it would be a copy, and the call would write that)"""
    import torch
    td, fd, _ = O.combo_types(combo)
    m, n, every, first = 64, 400, 3, 1
    x = signal(n, td, 4)
    bank = in_fd(random_bands(m), fd)
    nbands = bank[0].size
    rows = len(range(first, n, every))
    tdt = getattr(torch, np.dtype(fd).name)
    with make(m, "hann", combo) as p:
        p.set_filterbank(*bank)
        want = p.band_peak(x, every, first)
        # numpy
        out = np.full((rows, nbands, 2), -1.0, dtype=fd)
        p.reset()
        assert p.band_peak(x, every, first, out=out) is out and same_pairs(out, want)
        wide = np.full((rows, nbands, 4), -1.0, dtype=fd)
        before = p.state()
        with pytest.raises(ValueError):
            p.band_peak(x, every, first, out=wide[:, :, ::2])
        assert (wide == -1.0).all() and same_state_of(p, before)
        # device tensors
        dx = to_dev(x)
        out = torch.full((rows, nbands, 2), -1.0, dtype=tdt, device="cuda")
        p.reset()
        assert p.band_peak(dx, every, first, out=out) is out and same_pairs(out, want)
        before = p.state()
        for view in (torch.full((rows, nbands, 4), -1.0, dtype=tdt, device="cuda")[:, :, ::2],
                     torch.full((nbands, rows, 2), -1.0, dtype=tdt, device="cuda").permute(1, 0, 2)):
            assert tuple(view.shape) == (rows, nbands, 2) and not view.is_contiguous()
            with pytest.raises(ValueError):
                p.band_peak(dx, every, first, out=view)
            assert bool((view == -1.0).all()) and same_state_of(p, before)
        with pytest.raises(ValueError):                      # a numpy out for device samples
            p.band_peak(dx, every, first, out=np.zeros((rows, nbands, 2), dtype=fd))


def same_state_of(p, before):
    after = p.state()
    return all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]


def test_band_peak_errors_leave_state_and_filterbank_untouched():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    with make(m, "hann", combo) as p:
        api = p.api
        out = np.zeros((10, m, 2), dtype=np.float32)
        # no filterbank installed
        api.clear()
        assert p.filterbank_bands == 0
        assert api.sdft_band_peak_n(p._p, 100, x.ctypes.data, 10, 0, out.ctypes.data) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_band_peak_n" in err and "filterbank" in err, err
        api.clear()
        with pytest.raises(ValueError):
            p.band_peak(x[:10])
        bank = in_fd(random_bands(m), np.float32)
        p.set_filterbank(*bank)
        nbands = bank[0].size
        p.band_peak(x[:300])                                  # (errors against a plan that is mid-stream)
        before = p.state()
        with make(m, "hann", combo) as q:                     # what the installed filterbank gives from here on
            q.set_filterbank(*bank)
            q.band_peak(x[:300])
            want = q.band_peak(x[300:900], 7, 2)

        def untouched(what):
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], what
            assert p.filterbank_bands == nbands, what

        big = np.zeros((10, nbands, 2), dtype=np.float32)
        for n, every, ptr, word in [(100, 0, big.ctypes.data, "every"), (100, 10, None, "NULL")]:
            api.clear()
            assert api.sdft_band_peak_n(p._p, n, x.ctypes.data, every, 0, ptr) == -1, word
            err = api.last_error()
            assert err and "sdft_hip_sdft_band_peak_n" in err and word in err, err
            api.clear()
            untouched(word)
        # n == 0: no rows, nothing moves
        assert api.sdft_band_peak_n(p._p, 0, x.ctypes.data, 10, 0, None) == 0 and api.last_error() is None
        untouched("n == 0")
        # the installed filterbank still answers as before
        assert same_pairs(p.band_peak(x[300:900], 7, 2), want)
        # first >= n: no row kept, peaks may be NULL, the stream only advances
        assert api.sdft_band_peak_n(p._p, 400, x[900:1300].ctypes.data, 10, 400, None) == 0 and api.last_error() is None
        assert p.state()[3] != before[3]
        with make(m, "hann", combo) as q:
            q.set_filterbank(*bank)
            q.sdft(x[:1300])
            assert same_state(p, q)
        assert p.band_peak(x[1300:1700], 10, 400).shape == (0, nbands, 2)
        # no bands: the filterbank is removed
        p.set_filterbank([], [], [])
        api.clear()
        assert api.sdft_band_peak_n(p._p, 100, x.ctypes.data, 10, 0, big.ctypes.data) == -1
        api.clear()


# ---------------------------------------------------------------------------------------------
# (15) a plain C host and a C++ host
# ---------------------------------------------------------------------------------------------
def host_bank(m, nbands, fd):
    """the hosts' filterbank (host_band_peak.c / .cpp): overlapping bands, wider than a tile"""
    start = np.arange(nbands) * m // 32
    length = np.minimum(m // 8 + 7 * np.arange(nbands), m - start)
    w = np.concatenate([(1 + (b * 31 + np.arange(length[b]) * 7) % 13) / 16 - 0.25 for b in range(nbands)])
    return in_fd((start.astype(np.uint64), length.astype(np.uint64), w), fd)


def check_host_rows(rows_file, combo, m, n, every, x, nbands=24):
    td, fd, _ = O.combo_types(combo)
    got = np.fromfile(rows_file, dtype=fd).reshape(-1, nbands, 2)
    bank = host_bank(m, nbands, fd)
    with make(m, "hann", combo) as p:
        p.set_filterbank(*bank)
        tiles, per = geometry(p)
        assert (pieces_of(bank, per) > 1).sum() > nbands // 2
        want = p.band_peak(x, every, 0)
    assert got.shape == want.shape
    b0, nb = bank[0].astype(np.int64), bank[1].astype(np.int64)
    assert ((got[..., 1] >= b0) & (got[..., 1] < b0 + nb)).all()
    if exact_combo(combo):
        assert same_pairs(got, want)


@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_band_peak(tmp_path, hip_library, flags, combo):
    """tests/c/host_band_peak.c: a stream in calls of ragged lengths, each with the documented next first, and the error returns
    through sdft_hip_last_error; its rows against SDFT.band_peak of the whole signal in one call (FD float: bit for bit)"""
    td = O.combo_types(combo)[0]
    exe = tmp_path / "host_band_peak"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_band_peak.c"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every = 1000, 6000, 7
    x = signal(n, td, m)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(tmp_path / "x.raw"), str(tmp_path / "rows.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-BAND-PEAK ok" in r.stdout
    check_host_rows(tmp_path / "rows.raw", combo, m, n, every, x)


@pytest.mark.parametrize("t,f,combo", [("float", "double", "f32f64"), ("double", "double", "f64f64"), ("float", "float", "f32f32")])
def test_cpp_facade_band_peak(tmp_path, hip_library, t, f, combo):
    """tests/cpp/host_band_peak.cpp: sdft::SDFT<T, F>::band_peak for the type pairs of test_cpp_facade_host; the host checks one-bin
    bands against power() bit for bit with bin k and a whole-row band against the largest power, and writes the rows of a ragged
    stream, compared here with SDFT.band_peak of the whole signal (FD float: bit for bit)"""
    td = O.combo_types(combo)[0]
    exe = tmp_path / "host_band_peak_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", f"-DHOST_T={t}", f"-DHOST_F={f}", "-I", os.path.join(ROOT, "include", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_band_peak.cpp"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every = 1000, 6000, 7
    x = signal(n, td, 9)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(tmp_path / "x.raw"), str(tmp_path / "rows.raw")], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0 and "CPP-BAND-PEAK ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    check_host_rows(tmp_path / "rows.raw", combo, m, n, every, x)
