"""Filterbank analysis (sdft_hip_set_filterbank, sdft_hip_sdft_filterbank_n, SDFT.filterbank) on a real MI355X against the oracle.

The expected powers are those of tests/test_gpu_power.py: the oracle fed in blocks, re*re + im*im of its rows kept in the FD
dtype, never a complex matrix.  With W the dense band matrix, the reference value is W @ p and T = |W| @ p, both in float64
(on the device: the products of a parity case are 10^12).  The bars are the contract's, element by element, L the band's bin
count, u = 2^-24 / 2^-53, gamma_n = n u / (1 - n u), eta the smallest positive subnormal of the FD type:
    FD float    gamma_(L+1) T + L eta      float64 products are exact and the float64 sum's own error is below 2^-28 T
    FD double   2 gamma_L T + L eta        the float64 evaluation itself errs by up to gamma_L T
and on the inexact route (FD double with the default carries) the power call's term deviation on top: BAR of
tests/test_gpu_power.py (2.1e-11) times the largest power on the call's grid times sum |w|.  Every element of every row is compared."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd import filterbank as F
from test_gpu_power import BAR, ROOT, WINDOWS, MS, exact_combo, expected, make, on_grid, power_of, rel, signal, to_dev

pytestmark = pytest.mark.gpu
GRIDS = [(1, 0), (7, 6), (100, 0), (1024, 1023)]


# ---------------------------------------------------------------------------------------------
# filterbanks
# ---------------------------------------------------------------------------------------------
def whole_row(m):
    return np.array([0], dtype=np.uint64), np.array([m], dtype=np.uint64), np.ones(m)


def one_bin_bands(m):
    return np.arange(m, dtype=np.uint64), np.ones(m, dtype=np.uint64), np.ones(m)


def random_bands(m, seed=None):
    """3 m bands (more bands than bins): starts over the whole row, lengths from 1 to m (band 0 is the whole row, band 1 one bin),
    bands that straddle the bins 61/62 and 123/124 (the first tile boundaries at 62 bins per tile and at 2 x 62), weights drawn from
    {0, 1, -0.5, uniform in [2^-10, 1]}"""
    rng = np.random.default_rng(1000 + m if seed is None else seed)
    nb = 3 * m
    start = rng.integers(0, m, nb)
    length = 1 + (rng.random(nb) * rng.random(nb) * (m - start)).astype(np.int64)      # short bands are the many, long ones the few
    length = np.minimum(length, m - start)
    start[0], length[0] = 0, m
    start[1], length[1] = m - 1, 1
    fixed = [b for b in ((61, 2), (60, 4), (123, 2), (120, 8), (61, 63)) if b[0] + b[1] <= m]
    for i, (s, k) in enumerate(fixed):
        start[2 + i], length[2 + i] = s, k
    assert (length >= 1).all() and (start + length <= m).all() and length.max() == m
    total = int(length.sum())
    kind = rng.integers(0, 4, total)
    w = np.choose(kind, [np.zeros(total), np.ones(total), np.full(total, -0.5), rng.uniform(2.0 ** -10, 1.0, total)])
    return start.astype(np.uint64), length.astype(np.uint64), w


def banks_of(m):
    banks = [("whole row", whole_row(m)), ("one-bin bands", one_bin_bands(m)), ("random", random_bands(m))]
    if m >= 64:
        banks.append(("mel", F.mel(m, 48000, min(40, m))))
    return banks


def in_fd(bank, fd):
    """the weights as the plan holds them (rounded to the FD type once, here)"""
    return bank[0], bank[1], np.asarray(bank[2]).astype(fd)


# ---------------------------------------------------------------------------------------------
# reference and bars
# ---------------------------------------------------------------------------------------------
def reference(bank, p64):
    """(W @ p, |W| @ p, L, sum |w|) for the rows of p64 (a float64 device tensor [rows][m]); W from the FD weights"""
    import torch
    W = torch.from_numpy(F.dense(p64.shape[1], *bank).astype(np.float64)).cuda()
    R = p64 @ W.T
    T = p64 @ W.abs().T
    L = torch.from_numpy(np.asarray(bank[1]).astype(np.float64)).cuda()
    return R, T, L, W.abs().sum(dim=1)


def bar_of(fd, T, L, sum_w, inexact_scale):
    single = np.dtype(fd) == np.float32
    u = 2.0 ** -24 if single else 2.0 ** -53
    eta = 2.0 ** -149 if single else 5e-324
    if single:
        gamma = (L + 1) * u / (1 - (L + 1) * u)
        bar = gamma * T + L * eta
    else:
        gamma = L * u / (1 - L * u)
        bar = 2 * gamma * T + L * eta
    if inexact_scale:
        bar = bar + BAR * inexact_scale * sum_w
    return bar


def check_rows(got, R, T, L, sum_w, fd, inexact_scale, what):
    import torch
    got = got if hasattr(got, "cpu") else torch.from_numpy(got).cuda()
    assert tuple(got.shape) == tuple(R.shape) and got.dtype == getattr(torch, np.dtype(fd).name), (what, got.shape, R.shape, got.dtype)
    err = (got.double() - R).abs()
    bar = bar_of(fd, T, L, sum_w, inexact_scale)
    bad = ~(err <= bar)                                       # (a NaN fails)
    worst = float((err / torch.clamp(bar, min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: largest error / bar = {worst:.3g}")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x filterbank x grid
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("m", MS)
def test_filterbank_parity(m, window, combo):
    import torch
    fd = O.combo_types(combo)[1]
    n = 10000 if m == 4096 else 6000            # several chunks, and a roll-over at 2N
    x, want = expected(combo, window, m, n)
    dx = to_dev(x)
    p64 = torch.from_numpy(np.array(want)).cuda().double()
    with make(m, window, combo) as p:
        for b, (name, bank) in enumerate(banks_of(m)):
            bank = in_fd(bank, fd)
            p.set_filterbank(*bank)
            assert p.filterbank_bands == bank[0].size
            R, T, L, sum_w = reference(bank, p64)
            for g, (every, first) in enumerate(GRIDS):
                p.reset()
                got = p.filterbank(dx if (b + g) % 2 else x, every, first)          # host and device memory alternate
                assert p.get_option("last_kernel") == 7, (m, name, every, first)
                if m >= 1000:
                    assert p.get_option("last_chunks") > 1, (m, name, every, first)
                inexact = 0.0 if exact_combo(combo) else float(p64[first::every].max())
                check_rows(got, R[first::every], T[first::every], L, sum_w, fd, inexact, (combo, window, m, name, every, first))
                del got
            del R, T


# ---------------------------------------------------------------------------------------------
# bit-exact cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_one_bin_bands_are_the_power_call(combo):
    """dftsize one-bin bands of weight 1 against SDFT.power of the same call on a twin plan with the same options, bit for bit on
    every route: one chunk, chunk-parallel (default FD double: the inexact route, where both calls make the same chunks), exact
    carries, host and device memory"""
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
                got, want = p.filterbank(xs, every, first), q.power(xs, every, first)
                assert p.get_option("last_kernel") == 7 and q.get_option("last_kernel") == 5
                assert p.get_option("last_chunks") == q.get_option("last_chunks")
                got, want = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (got, want))
                assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (combo, m, every, first)


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f64f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {"carry": 1})])
def test_two_bin_bands_are_two_rounded_products_and_their_sum(combo, opts):
    """bands (k, 2) for every k, tile boundaries included, on the routes that are bit-identical to the reference: exactly numpy's
    w0 * p0 + w1 * p1 in the FD dtype"""
    td, fd, _ = O.combo_types(combo)
    for m in (2, 125, 1000):
        n = 6000
        x, pw = expected(combo, "hann", m, n)
        rng = np.random.default_rng(m)
        w = rng.uniform(-1.0, 1.0, (m - 1, 2)).astype(fd)
        with make(m, "hann", combo, **opts) as p:
            p.set_filterbank(np.arange(m - 1), np.full(m - 1, 2), w.ravel())
            for i, (every, first) in enumerate(((1, 0), (100, 37))):
                p.reset()
                got = p.filterbank(to_dev(x) if i else x, every, first)
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                rows = on_grid(pw, every, first)
                want = w[:, 0] * rows[:, :-1] + w[:, 1] * rows[:, 1:]
                assert want.dtype == fd and np.array_equal(got, want), (combo, m, every, first)


# ---------------------------------------------------------------------------------------------
# streaming, chunking, state, determinism
# ---------------------------------------------------------------------------------------------
EXACT = [("f32f32", {}), ("f64f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {"carry": 1})]


@pytest.mark.parametrize("combo,opts", EXACT)
def test_filterbank_streaming_and_chunking_bit_identical(combo, opts):
    """one call of n samples against calls of ragged lengths chained by the documented next first: the same rows and the same final
    state, bit for bit; and the one call with option chunk forced to two other values: the same rows (a row's bits do not depend
    on the time chunking)"""
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
            whole = p.filterbank(to_dev(x), every, 0).cpu().numpy()
            chunks = p.get_option("last_chunks")
            assert chunks > 1
            got, t, first = [], 0, 0
            for i, k in enumerate(lengths):
                xs = x[t:t + k]
                d = q.filterbank(to_dev(xs) if i % 2 else xs, every, first)
                got.append(d.cpu().numpy() if hasattr(d, "cpu") else d)
                first = every_next_first(k, every, first)
                t += k
            assert np.array_equal(np.concatenate(got), whole), (combo, every)
            for a, b in zip(p.state()[:3], q.state()[:3]):
                assert np.array_equal(a, b), (combo, every)
            assert p.state()[3] == q.state()[3]
            for forced in (256, 1024):
                p.reset()
                p.set_option("chunk", forced)
                again = p.filterbank(to_dev(x), every, 0).cpu().numpy()
                assert p.get_option("last_chunks") not in (1, chunks), (forced, chunks)
                assert np.array_equal(again, whole), (combo, every, forced)
            p.set_option("chunk", 0)


@pytest.mark.parametrize("combo", O.COMBOS)
def test_state_after_a_filterbank_call_is_sdft_n_s(combo):
    """sdft_sdft_n of further samples gives, after a filterbank call, the rows it gives after sdft_sdft_n of the same prefix"""
    td, fd, _ = O.combo_types(combo)
    m, n, more = 1000, 6000, 700
    x = signal(n + more, td, 31)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        p.set_filterbank(*in_fd(F.mel(m, 48000, 40), fd))
        p.filterbank(to_dev(x[:n]), 100, 5)
        q.sdft(to_dev(x[:n]))
        a, b = p.sdft(x[n:]), q.sdft(x[n:])
        if exact_combo(combo):
            assert np.array_equal(a, b)
        else:
            assert rel(a, b) <= 1e-11, rel(a, b)
        assert p.state()[3] == q.state()[3]


@pytest.mark.parametrize("combo", O.COMBOS)
def test_filterbank_is_deterministic(combo):
    td, fd, _ = O.combo_types(combo)
    m, n = 1024, 6000
    x = signal(n, td, 41)
    bank = in_fd(random_bands(m), fd)
    outs = []
    for _ in range(2):
        with make(m, "blackman", combo) as p:
            p.set_filterbank(*bank)
            outs.append(p.filterbank(to_dev(x), 3, 1).cpu().numpy())
            assert p.get_option("last_chunks") > 1
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f32f64", {"carry": 1})])
def test_filterbank_batched_channels(combo, opts):
    """a 3-channel plan, out [3][rows][nbands], against three single-channel plans, bit for bit (on the routes whose values do not
    depend on the time chunks, which the channel count changes)"""
    td, fd, _ = O.combo_types(combo)
    ch, m, n = 3, 256, 6000
    x = np.stack([signal(n, td, 200 + c) for c in range(ch)])
    bank = in_fd(random_bands(m), fd)
    for device in (False, True):
        for every, first in ((100, 50), (3, 1)):
            with make(m, "blackman", combo, channels=ch, **opts) as p:
                p.set_filterbank(*bank)
                got = p.filterbank(to_dev(x) if device else x, every, first)
                got = got.cpu().numpy() if device else got
                assert p.get_option("last_kernel") == 7
            assert got.shape[0] == ch and got.shape[2] == bank[0].size
            for c in range(ch):
                with make(m, "blackman", combo, **opts) as q:
                    q.set_filterbank(*bank)
                    assert np.array_equal(got[c], q.filterbank(x[c], every, first)), (combo, device, every, c)


# ---------------------------------------------------------------------------------------------
# no overrun, no hole, at the least alignment an element allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_filterbank_guarded_misaligned_output(combo, host):
    """out carved from a guarded arena at residue sizeof(fd) of a 16-byte address, an odd number of bands (consecutive rows change
    alignment), split bands among them"""
    import torch
    td, fd, _ = O.combo_types(combo)
    m, n, every, first = 1000, 2000, 3, 1
    x, p_all = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    bank = (bank[0][:-1], bank[1][:-1], bank[2][:int(bank[1][:-1].sum())])
    nbands = bank[0].size
    assert nbands % 2 == 1
    rows = on_grid(p_all, every, first).shape[0]
    size = np.dtype(fd).itemsize
    R, T, L, sum_w = reference(bank, torch.from_numpy(np.array(on_grid(p_all, every, first))).cuda().double())
    with make(m, "hann", combo) as p:
        p.set_filterbank(*bank)
        arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, nbands), fd)))
        xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
        out = arena.carve((rows, nbands), fd, size, 16, name="out")
        assert G.ptr_of(out) % 16 == size
        p.api.clear()
        got = p.api.sdft_filterbank_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, C.c_void_p(G.ptr_of(out)))
        p.synchronize()
        assert got == rows, p.api.last_error()
        assert p.get_option("last_kernel") == 7 and p.get_option("last_chunks") > 1
        arena.check()
        assert G.view_unwritten(out) == 0
        assert np.array_equal(G.to_numpy(xv), x)
        inexact = 0.0 if exact_combo(combo) else float(on_grid(p_all, every, first).max())
        check_rows(np.ascontiguousarray(G.to_numpy(out)), R, T, L, sum_w, fd, inexact, (combo, host))


# ---------------------------------------------------------------------------------------------
# calls whose pieces exceed the workspace bound: several forward launches, each followed by the rows kernel on its rows
# ---------------------------------------------------------------------------------------------
FB_BOUND = 64 << 20                                          # logic::kFilterbankWorkspaceBytes, as sdft_hip.h and DESIGN.md state it
BOUNDED = [("f32f32", {}), ("f32f64", {"carry": 1})]         # the routes on which a row's bits do not depend on the time chunks


def same_bits(a, b):
    import torch
    if hasattr(a, "cpu") and hasattr(b, "cpu"):              # (on the device: these matrices are tens of MB)
        iv = torch.int32 if a.dtype == torch.float32 else torch.int64
        return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(iv), b.contiguous().view(iv)))
    a, b = (np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_state(p, q):
    a, b = p.state(), q.state()
    return all(same_bits(u, v) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]


def geometry(p):
    """(tiles, bins a tile owns) of a plan"""
    return p.get_option("tiles"), p.get_option("interior") * p.get_option("bins_per_lane")


def four_tile_plan(combo, channels=1, **opts):
    """a plan of 256 bins, or of the fewest bins that make 4 tiles"""
    p = make(256, "hann", combo, channels, **opts)
    tiles, per = geometry(p)
    if tiles < 4:
        p.close()
        p = make(3 * per + 1, "hann", combo, channels, **opts)
    assert p.get_option("tiles") >= 4
    return p


def pieces_of(bank, per):
    """pieces per band: the tiles it has bins in"""
    b0, nb = np.asarray(bank[0]).astype(np.int64), np.asarray(bank[1]).astype(np.int64)
    return (b0 + nb - 1) // per - b0 // per + 1


def slots_of(bank, per):
    """workspace slots per row and channel: the pieces of the split bands (logic::filterbank_layout)"""
    k = pieces_of(bank, per)
    return int(k[k > 1].sum())


def split_bank(m, tiles, per, nslots, exact=False, seed=7):
    """Split bands of at least nslots workspace slots (exact: of nslots), one unsplit band to four of them, in shuffled order.  The
    split bands repeat one set: for every piece count 2 ... tiles and every first tile a band from the tile's first bin to the first
    bin of its last tile (it starts and ends on a boundary bin), one from the last bin before a boundary to its last tile's last
    bin, and one with both ends drawn.  The unsplit ones: a whole tile, one bin, a drawn range.  Weights as random_bands."""
    rng = np.random.default_rng(seed)

    def split_set():
        out = []
        for k in range(2, tiles + 1):
            for t0 in range(tiles - k + 1):
                t1 = t0 + k - 1
                a0, a1 = t0 * per, (t0 + 1) * per                          # the bins [a0, a1) of the first tile
                b0, b1 = t1 * per, min((t1 + 1) * per, m)                   # ... of the last
                out.append((a0, b0 + 1 - a0))
                out.append((a1 - 1, b1 - (a1 - 1)))
                s, e = int(rng.integers(a0, a1)), int(rng.integers(b0, b1))
                out.append((s, e + 1 - s))
        return out

    bands, slots = [], 0
    while slots < nslots:
        for s, k in split_set():
            pieces, left = (s + k - 1) // per - s // per + 1, nslots - slots
            if left <= 0:
                break
            if exact and left != pieces and left - pieces < 2:              # (what stays can still be made of bands of 2 and 3 pieces)
                continue
            bands.append((s, k))
            slots += pieces
    for i in range(len(bands) // 4 + tiles):
        t = int(rng.integers(0, tiles))
        a0, a1 = t * per, min((t + 1) * per, m)
        s = int(rng.integers(a0, a1))
        bands.append([(a0, a1 - a0), (s, 1), (s, int(rng.integers(s, a1)) + 1 - s)][i % 3])
    bands = np.array(bands, dtype=np.int64)[rng.permutation(len(bands))]
    start, length = bands[:, 0], bands[:, 1]
    assert (length >= 1).all() and (start + length <= m).all()
    total = int(length.sum())
    kind = rng.integers(0, 4, total)
    w = np.choose(kind, [np.zeros(total), np.ones(total), np.full(total, -0.5), rng.uniform(2.0 ** -10, 1.0, total)])
    bank = start.astype(np.uint64), length.astype(np.uint64), w
    k = pieces_of(bank, per)
    assert set(k.tolist()) == set(range(1, tiles + 1)), sorted(set(k.tolist()))          # every piece count, 1 = unsplit
    assert ((start % per == 0) & (k > 1)).any() and (((start + length) % per == 0) & (k > 1)).any()
    assert slots_of(bank, per) == nslots if exact else slots_of(bank, per) >= nslots
    split = k > 1
    assert (split[1:] != split[:-1]).sum() > len(k) // 8                                  # direct and workspace stores alternate
    return bank


def launches_needed(channels, rows, nslots, size):
    return -(-(channels * rows * nslots * size) // FB_BOUND)


def run_beyond_the_bound(combo, opts, n, every, first):
    """One device call whose pieces are at least 3 x 64 MiB, against the float64 W @ p, and bit for bit (rows and final state)
    against a twin plan fed the same samples in calls of one launch each.  Returns (rows, launches, chunks)."""
    import torch
    from sdft_amd.sdft import every_next_first, every_rows
    td, fd, _ = O.combo_types(combo)
    size = np.dtype(fd).itemsize
    rows = every_rows(n, every, first)
    with four_tile_plan(combo, **opts) as p, four_tile_plan(combo, **opts) as q:
        m = p.dftsize
        tiles, per = geometry(p)
        bank = in_fd(split_bank(m, tiles, per, -(-3 * FB_BOUND // (rows * size))), fd)
        nslots = slots_of(bank, per)
        assert rows * nslots * size >= 3 * FB_BOUND
        x, pw = expected(combo, "hann", m, n)
        p.set_filterbank(*bank); q.set_filterbank(*bank)
        got = p.filterbank(to_dev(x), every, first)
        launches, chunks = p.get_option("last_filterbank_launches"), p.get_option("last_chunks")
        print(f"{(combo, m, n, every, first)}: {bank[0].size} bands, {nslots} slots, {chunks} chunks in {launches} launches")
        assert p.get_option("last_kernel") == 7 and chunks > 1
        assert launches >= launches_needed(1, rows, nslots, size)
        assert 3 <= launches < chunks                        # several chunks to a launch, and the last launch ragged
        R, T, L, sum_w = reference(bank, torch.from_numpy(np.array(on_grid(pw, every, first))).cuda().double())
        check_rows(got, R, T, L, sum_w, fd, 0.0, ("beyond the bound", combo, m, n, every, first))
        del R, T
        # the same samples in calls whose rows fit the workspace
        fit = FB_BOUND // (nslots * size)                    # rows of one launch
        lengths = [1, 511, 512, 513]
        while sum(lengths) < n:
            lengths.append(min(fit * every - 5, n - sum(lengths)))
        parts, t, f = [], 0, first
        for k in lengths:
            parts.append(q.filterbank(to_dev(x[t:t + k]), every, f))
            assert q.get_option("last_filterbank_launches") == 1, (k, f)
            f = every_next_first(k, every, f)
            t += k
        assert same_bits(torch.cat(parts), got), (combo, every, first)
        assert same_state(p, q), (combo, every, first)
    return rows, launches, chunks


@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_filterbank_beyond_the_workspace_bound(combo, opts):
    """(every, first) = (1, 0): launches begin at rows that are multiples of the chunk length"""
    run_beyond_the_bound(combo, opts, 6000, 1, 0)


@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_filterbank_beyond_the_workspace_bound_on_a_sparse_grid(combo, opts):
    """(every, first) = (3, 2): a chunk of 128 samples keeps 42 or 43 rows, launches begin wherever those add up to"""
    run_beyond_the_bound(combo, opts, 6000, 3, 2)


@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_filterbank_beyond_the_workspace_bound_by_channels_alone(combo, opts):
    """4096 rows x slots = 64 MiB exactly: one launch for one channel, three channels exceed the bound by their count alone (the
    workspace is [channels][rows of the launch][slots], the channel stride changes from launch to launch).  Every channel against
    its single-channel plan, bit for bit; channel 0 against the reference as well."""
    import torch
    td, fd, _ = O.combo_types(combo)
    size = np.dtype(fd).itemsize
    ch, n = 3, 4096
    nslots = FB_BOUND // (n * size)
    assert n * nslots * size == FB_BOUND
    with four_tile_plan(combo, ch, **opts) as p:
        m = p.dftsize
        tiles, per = geometry(p)
        bank = in_fd(split_bank(m, tiles, per, nslots, exact=True), fd)
        x0, pw = expected(combo, "hann", m, n)
        x = np.stack([x0] + [signal(n, td, 300 + c) for c in range(1, ch)])
        p.set_filterbank(*bank)
        got = p.filterbank(to_dev(x), 1, 0)
        launches, chunks = p.get_option("last_filterbank_launches"), p.get_option("last_chunks")
        assert p.get_option("last_kernel") == 7
        assert ch * n * nslots * size >= 3 * FB_BOUND and launches >= launches_needed(ch, n, nslots, size)
        assert 3 <= launches < chunks
    R, T, L, sum_w = reference(bank, torch.from_numpy(np.array(pw)).cuda().double())
    check_rows(got[0], R, T, L, sum_w, fd, 0.0, ("three channels, channel 0", combo, m))
    del R, T
    for c in range(ch):
        with four_tile_plan(combo, **opts) as q:
            q.set_filterbank(*bank)
            one = q.filterbank(to_dev(x[c]), 1, 0)
            assert q.get_option("last_filterbank_launches") == 1
            assert same_bits(got[c], one), (combo, c)


@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_filterbank_one_chunk_beyond_the_workspace_bound(combo, opts):
    """chunk = 1024 with more than 64 MiB / 1024 slots: a launch is one chunk and the workspace grows past its bound; the rows of
    the call with the library's own chunks (several to a launch), bit for bit"""
    import torch
    td, fd, _ = O.combo_types(combo)
    size = np.dtype(fd).itemsize
    n, forced = 3000, 1024
    with four_tile_plan(combo, chunk=forced, **opts) as p, four_tile_plan(combo, **opts) as q:
        m = p.dftsize
        tiles, per = geometry(p)
        bank = in_fd(split_bank(m, tiles, per, max(-(-3 * FB_BOUND // (n * size)), FB_BOUND // (forced * size) + 1)), fd)
        nslots = slots_of(bank, per)
        assert forced * nslots * size > FB_BOUND and n * nslots * size >= 3 * FB_BOUND
        x, pw = expected(combo, "hann", m, n)
        p.set_filterbank(*bank); q.set_filterbank(*bank)
        got = p.filterbank(to_dev(x), 1, 0)
        assert p.get_option("last_kernel") == 7 and p.get_option("last_chunk_len") == forced
        assert p.get_option("last_filterbank_launches") == p.get_option("last_chunks") == -(-n // forced)
        R, T, L, sum_w = reference(bank, torch.from_numpy(np.array(pw)).cuda().double())
        check_rows(got, R, T, L, sum_w, fd, 0.0, ("one chunk beyond the bound", combo, m))
        del R, T
        want = q.filterbank(to_dev(x), 1, 0)
        assert 3 <= q.get_option("last_filterbank_launches") < q.get_option("last_chunks")
        assert same_bits(got, want), combo
        assert same_state(p, q), combo


def test_filterbank_beyond_the_workspace_bound_chunk_parallel_carries():
    """FD double with its default carries (the inexact route), several launches: the contract's bar with the inexact term, and
    the same bytes from two fresh plans"""
    import torch
    combo, n = "f64f64", 6000
    td, fd, _ = O.combo_types(combo)
    outs = []
    for _ in range(2):
        with four_tile_plan(combo) as p:
            m = p.dftsize
            tiles, per = geometry(p)
            bank = in_fd(split_bank(m, tiles, per, -(-3 * FB_BOUND // (n * 8))), fd)
            nslots = slots_of(bank, per)
            assert n * nslots * 8 >= 3 * FB_BOUND
            x, pw = expected(combo, "hann", m, n)
            p.set_filterbank(*bank)
            outs.append(p.filterbank(to_dev(x), 1, 0))
            launches = p.get_option("last_filterbank_launches")
            assert p.get_option("last_kernel") == 7 and launches >= launches_needed(1, n, nslots, 8)
            assert 3 <= launches < p.get_option("last_chunks")
    p64 = torch.from_numpy(np.array(pw)).cuda().double()
    R, T, L, sum_w = reference(bank, p64)
    check_rows(outs[0], R, T, L, sum_w, fd, float(p64.max()), ("beyond the bound, chunk-parallel carries", combo, m))
    assert same_bits(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------
# forced routes, host staging in segments, asynchronous calls
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(chunk=128), dict(chunk=1000), dict(carry=1, segments=3), dict(carry=1, chain=2), dict(carry=1, chain=0)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_filterbank_forced_routes(opts):
    """the option sets of test_power_sum_forced_routes; with exact carries the rows of the default exact route, bit for bit.  The
    kernel polls for no relay carries: whatever the options, the call never takes the flow form."""
    import torch
    combo, m, n = "f32f64", 1000, 6000
    fd = np.float64
    exact = "carry" in opts
    x, pw = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    p64 = torch.from_numpy(np.array(pw)).cuda().double()
    R, T, L, sum_w = reference(bank, p64)
    with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, carry=1) as q:
        p.set_filterbank(*bank); q.set_filterbank(*bank)
        for every, first in ((1, 0), (100, 37)):
            p.reset(); q.reset()
            got = p.filterbank(to_dev(x), every, first)
            assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 7 and p.get_option("last_flow") == 0
            if "chunk" in opts:
                assert p.get_option("last_chunk_len") == opts["chunk"]
            if "segments" in opts:
                assert p.get_option("last_segments") == opts["segments"]
            if "chain" in opts:
                assert p.get_option("last_chain") == (3 if opts["chain"] else 0)
            inexact = 0.0 if exact else float(p64[first::every].max())
            check_rows(got, R[first::every], T[first::every], L, sum_w, fd, inexact, ("forced route", opts, every, first))
            if exact:
                assert same_bits(got, q.filterbank(to_dev(x), every, first)), (opts, every, first)
                assert same_state(p, q), (opts, every, first)


def test_filterbank_beyond_the_workspace_bound_in_carry_segments():
    """segments = 3 with pieces of 3 x 64 MiB: the launches of the workspace bound nest inside the carry segments (a launch never
    spans two of them), more launches than segments"""
    import torch
    combo, n = "f32f64", 6000
    fd = np.float64
    with four_tile_plan(combo, carry=1, segments=3) as p, four_tile_plan(combo, carry=1) as q:
        m = p.dftsize
        tiles, per = geometry(p)
        bank = in_fd(split_bank(m, tiles, per, -(-3 * FB_BOUND // (n * 8))), fd)
        nslots = slots_of(bank, per)
        assert n * nslots * 8 >= 3 * FB_BOUND
        x, pw = expected(combo, "hann", m, n)
        p.set_filterbank(*bank); q.set_filterbank(*bank)
        got = p.filterbank(to_dev(x), 1, 0)
        segments, launches = p.get_option("last_segments"), p.get_option("last_filterbank_launches")
        assert p.get_option("last_kernel") == 7 and p.get_option("last_flow") == 0
        assert segments > 1 and launches > segments and launches >= launches_needed(1, n, nslots, 8)
        R, T, L, sum_w = reference(bank, torch.from_numpy(np.array(pw)).cuda().double())
        check_rows(got, R, T, L, sum_w, fd, 0.0, ("beyond the bound in carry segments", combo, m))
        del R, T
        assert same_bits(got, q.filterbank(to_dev(x), 1, 0))
        assert q.get_option("last_segments") == 1
        assert same_state(p, q)


@pytest.mark.parametrize("combo,opts", [("f32f64", {}), ("f32f32", {}), ("f32f64", {"carry": 1})])
def test_filterbank_host_staging_in_segments(combo, opts):
    """stage_bytes of 7 and of 2 output rows: host samples with host and with device output, grids whose rows fall on the first
    and the last sample of a segment, before and after its end, and one row for all segments; on the exact routes the rows of the
    unstaged call, bit for bit"""
    import torch
    from sdft_amd.sdft import every_rows
    fd = O.combo_types(combo)[1]
    m, n = 1000, 6000
    exact = exact_combo(combo) or "carry" in opts
    x, pw = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    nbands = bank[0].size
    row = nbands * np.dtype(fd).itemsize
    p64 = torch.from_numpy(np.array(pw)).cuda().double()
    R, T, L, sum_w = reference(bank, p64)
    with make(m, "hann", combo, **opts) as q:
        q.set_filterbank(*bank)
        # (the third: 700 samples' bytes, less than a row's -- the samples go in segments too, whatever memory the rows go to)
        for stage, grids in [(7 * row, [(100, 37), (100, 0), (100, 99)]), (2 * row, [(1024, 1023), (6000, 0), (700, 0)]),
                             (700 * x.itemsize, [(100, 37), (700, 699)])]:
            with make(m, "hann", combo, stage_bytes=stage, **opts) as p:
                p.set_filterbank(*bank)
                for every, first in grids:
                    rows = every_rows(n, every, first)
                    inexact = 0.0 if exact else float(p64[first::every].max())
                    q.reset()
                    want = q.filterbank(to_dev(x), every, first)
                    p.reset()
                    got = p.filterbank(x, every, first)
                    assert p.get_option("last_kernel") == 7
                    check_rows(got, R[first::every], T[first::every], L, sum_w, fd, inexact, (combo, opts, stage // row, every, first, "host"))
                    assert not exact or same_bits(got, want.cpu().numpy()), (combo, stage // row, every, first, "host")
                    assert same_state(p, q) if exact else p.state()[3] == q.state()[3]
                    p.reset()
                    out = torch.zeros((rows, nbands), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
                    ret = p.api.sdft_filterbank_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, C.c_void_p(out.data_ptr()))
                    p.synchronize()
                    assert ret == rows, p.api.last_error()
                    check_rows(out, R[first::every], T[first::every], L, sum_w, fd, inexact, (combo, opts, stage // row, every, first, "host samples, device rows"))
                    assert not exact or same_bits(out, want), (combo, stage // row, every, first, "device rows")


def test_filterbank_async_device_pointers():
    import torch
    combo, m, n, every, first = "f32f64", 1000, 6000, 100, 37
    x, pw = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), np.float64)
    p64 = torch.from_numpy(np.array(on_grid(pw, every, first))).cuda().double()
    R, T, L, sum_w = reference(bank, p64)
    with make(m, "hann", combo, **{"async": 1}) as p:
        p.set_filterbank(*bank)
        got = p.filterbank(to_dev(x), every, first)
        p.synchronize()
        assert p.get_option("last_kernel") == 7
        check_rows(got, R, T, L, sum_w, np.float64, float(p64.max()), "async")


# ---------------------------------------------------------------------------------------------
# option "interior" changes the tiles after the filterbank was installed: the bands are cut again
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {})])
def test_filterbank_is_cut_again_when_the_tiles_change(combo, opts):
    import torch
    from sdft_amd.sdft import SDFT
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, other = 1024, 6000, 7, 6, 62
    exact = exact_combo(combo) or "carry" in opts
    x, pw = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    p64 = torch.from_numpy(np.array(on_grid(pw, every, first))).cuda().double()
    R, T, L, sum_w = reference(bank, p64)
    inexact = 0.0 if exact else float(p64.max())
    with SDFT(m, "hann", 1.0, combo, hooks=True) as p:
        for k, v in opts.items():
            p.set_option(k, v)
        assert p.get_option("test_hooks") == 1
        p.set_filterbank(*bank)
        tiles0, interior0 = p.get_option("tiles"), p.get_option("interior")
        outs = []
        for step, lanes in enumerate((interior0, other, interior0)):
            p.set_option("interior", lanes)
            assert p.get_option("interior") == lanes and (p.get_option("tiles") != tiles0) == (lanes != interior0)
            p.reset()
            outs.append(p.filterbank(to_dev(x) if step % 2 else x, every, first))
            assert p.get_option("last_kernel") == 7 and p.get_option("last_chunks") > 1
            assert p.filterbank_bands == bank[0].size
            check_rows(outs[-1], R, T, L, sum_w, fd, inexact, (combo, "interior", lanes))
        assert same_bits(outs[0], outs[2]), combo
    if exact:
        # one-bin bands installed under the default tiles, cut again for the other ones: still the power call
        with SDFT(m, "hann", 1.0, combo, hooks=True) as p, SDFT(m, "hann", 1.0, combo, hooks=True) as q:
            for k, v in opts.items():
                p.set_option(k, v); q.set_option(k, v)
            p.set_filterbank(*in_fd(one_bin_bands(m), fd))
            p.filterbank(x[:700], every, first)
            p.set_option("interior", other); q.set_option("interior", other)
            assert p.get_option("tiles") != tiles0
            p.reset()
            got, want = p.filterbank(to_dev(x), every, first), q.power(to_dev(x), every, first)
            assert p.get_option("last_kernel") == 7 and q.get_option("last_kernel") == 5
            assert same_bits(got, want), combo


# ---------------------------------------------------------------------------------------------
# the analysis entry points interleaved on one plan
# ---------------------------------------------------------------------------------------------
PAIR_LISTS = ([(3, 3)], [(2, 0), (1, 3)])                    # (what a batched run draws its pair list from, beside PAIRS)
# what a run with the covariance call draws its array from: a full group permuted, a padded group with two channels left to
# advance-only items, one channel with three
ARRAY_LISTS = ([3, 1, 0, 2], [2, 0], [1])


def run_interleaved(combo, opts, m, seed, channels=1, covariance=False):
    """The body of test_analysis_entry_points_interleaved_on_one_plan; channels > 1 (tests/test_gpu_cross_sum_routes.py): a batched
    plan, the samples signals(td, n, seed), cross_sum a sixth kind, every expectation per channel.  p and pool carry a pair list,
    drawn again before some calls and installed in both (installing a list does not touch the state); the cross-spectrum call is
    checked as the pooled power call is -- pool's own call with the same memory, bit for bit, the same time chunks -- and against
    the twin's rows: at every == 1, first == 0 the bits of numpy's unfused expression, elsewhere check_pairs' bar for an exact
    route.  The state compared after every call is that of all channels, the ones no pair names included.
    covariance = True (tests/test_gpu_covariance_routes.py; channels > 1): covariance is a seventh kind; p and pool carry an array
    as well, drawn again from ARRAY_LISTS before some calls and before every covariance call (the state stays), and the call is
    checked as the cross-spectrum call is, its pairs being the array's upper triangle.  The kinds are then a drawn order of equal
    shares, not independent draws, and a list no call has run on yet is drawn before the others: every kind has run, and the
    covariance call on every array, whatever the seed."""
    from sdft_amd.sdft import covariance_pairs, every_rows
    from test_gpu_cross_sum import PAIRS, check_pairs, signals, terms
    td, fd, _ = O.combo_types(combo)
    batched = channels > 1
    rng = np.random.default_rng(100 * m + seed)
    n = 12000
    special = [1, 2, 99, 100, 511, 512, 513, 2 * m - 1, 2 * m, 2 * m + 1]
    calls = int(rng.integers(25, 41))
    cuts = np.sort(rng.choice(np.arange(1, n - sum(special)), calls - len(special) - 1, replace=False))
    drawn = np.diff(np.concatenate([[0], cuts, [n - sum(special)]]))
    lengths = rng.permutation(np.concatenate([special, drawn]).astype(np.int64))
    assert lengths.size == calls and lengths.sum() == n and (lengths >= 1).all()
    x = signals(td, n, seed, channels) if batched else signal(n, td, 50 + seed)
    bank = in_fd(random_bands(m), fd)
    covariance = covariance and batched
    names = ("sdft", "every", "power", "power_sum", "filterbank") + (("cross_sum",) if batched else ()) + (("covariance",) if covariance else ())
    lists = (PAIRS,) + PAIR_LISTS
    seen, installed, arrays = set(), set(), set()
    order = rng.permutation(np.resize(np.arange(len(names)), calls)) if covariance else None

    def install(pairs, *plans):
        for q in plans:
            q.set_pairs([a for a, _ in pairs], [b for _, b in pairs])
            assert q.pairs == len(pairs)
        installed.add(tuple(pairs))
        return pairs

    def install_array(chan, *plans):
        for q in plans:
            q.set_array(chan)
            assert q.array_channels == len(chan)
        a, b = covariance_pairs(len(chan))
        return [(chan[i], chan[j]) for i, j in zip(a.tolist(), b.tolist())]

    def draw(seq, done=None):
        left = [s for s in seq if tuple(s) not in done] if covariance and done is not None else []
        return (left or seq)[int(rng.integers(0, len(left or seq)))]

    with make(m, "hann", combo, channels, **opts) as p, make(m, "hann", combo, channels, **opts) as twin, \
            make(m, "hann", combo, channels, **opts) as lone, make(m, "hann", combo, channels, **opts) as pool:
        p.set_filterbank(*bank); lone.set_filterbank(*bank)
        pairs = install(PAIRS, p, pool) if batched else None
        chan = ARRAY_LISTS[0]
        elements = install_array(chan, p, pool) if covariance else None
        t = 0
        for i, k in enumerate(lengths.tolist()):
            kind = names[int(order[i])] if covariance else names[int(rng.integers(0, len(names)))]
            every = int(rng.choice([1, 2, 3, 7, 100, int(rng.integers(1, 600))]))
            first = int(rng.integers(0, every + 2))
            b0 = int(rng.integers(0, m))
            band = (b0, int(rng.integers(1, m - b0 + 1)))
            cols = slice(band[0], band[0] + band[1])
            xs = np.ascontiguousarray(x[..., t:t + k])
            xin = to_dev(xs) if i % 2 else xs
            what = (combo, m, seed, i, kind, k, every, first, band)
            before = twin.state()
            rows = twin.sdft(xs)
            if batched and int(rng.integers(0, 3)) == 0:     # a list installed mid-stream: the state stays
                was = p.state()
                pairs = install(draw(lists, installed), p, pool)
                now = p.state()
                assert all(same_bits(u, v) for u, v in zip(was[:3], now[:3])) and was[3] == now[3], what
            if covariance and (kind == "covariance" or int(rng.integers(0, 3)) == 0):    # an array installed mid-stream: the state stays
                was = p.state()
                chan = draw(ARRAY_LISTS, arrays if kind == "covariance" else None)
                elements = install_array(chan, p, pool)
                now = p.state()
                assert all(same_bits(u, v) for u, v in zip(was[:3], now[:3])) and was[3] == now[3], what
            if kind == "sdft":
                got, want = p.sdft(xin), rows
            elif kind == "every":
                got, want = p.sdft_every(xin, every, first), rows[..., first::every, :]
            elif kind == "power":
                got, want = p.power(xin, every, first, bins=band), power_of(rows)[..., first::every, cols]
            elif kind == "power_sum":
                got, want = p.power_sum(xin, every, first, bins=band), pool.power_sum(xin, every, first, bins=band)
                assert (p.get_option("last_chunks"), p.get_option("last_chunk_len")) == (pool.get_option("last_chunks"), pool.get_option("last_chunk_len")), what
                if every == 1 and first == 0:
                    assert same_bits(got, np.ascontiguousarray(power_of(rows)[..., cols])), what
            elif kind == "cross_sum":
                got, want = p.cross_sum(xin, every, first, bins=band), pool.cross_sum(xin, every, first, bins=band)
                assert p.get_option("last_kernel") == 8 and pool.get_option("last_kernel") == 8, what
                assert (p.get_option("last_chunks"), p.get_option("last_chunk_len")) == (pool.get_option("last_chunks"), pool.get_option("last_chunk_len")), what
                host = got.cpu().numpy() if hasattr(got, "cpu") else got
                if every == 1 and first == 0:
                    for j, (a, b) in enumerate(pairs):
                        re, im = terms(rows[a][:, cols], rows[b][:, cols])
                        assert same_bits(host[j].real, re) and same_bits(host[j].imag, im), (what, (a, b))
                check_pairs(host, rows, pairs, k, every, first, band, True, what)
            elif kind == "covariance":
                got, want = p.covariance(xin, every, first, bins=band), pool.covariance(xin, every, first, bins=band)
                assert p.get_option("last_kernel") == 9 and pool.get_option("last_kernel") == 9, what
                assert (p.get_option("last_chunks"), p.get_option("last_chunk_len")) == (pool.get_option("last_chunks"), pool.get_option("last_chunk_len")), what
                host = got.cpu().numpy() if hasattr(got, "cpu") else got
                if every == 1 and first == 0:
                    for j, (a, b) in enumerate(elements):
                        re, im = terms(rows[a][:, cols], rows[b][:, cols])
                        assert same_bits(host[j].real, re) and same_bits(host[j].imag, im), (what, (a, b))
                check_pairs(host, rows, elements, k, every, first, band, True, what)
                arrays.add(tuple(chan))
            else:
                lone.set_state(*before)
                got, want = p.filterbank(xin, every, first), lone.filterbank(xs, every, first)
                assert got.shape == ((channels,) if batched else ()) + (every_rows(k, every, first), bank[0].size), what
            if kind not in ("power_sum", "cross_sum", "covariance"):
                pool.sdft(xs)
            assert same_bits(got, want if hasattr(want, "cpu") else np.ascontiguousarray(want)), what
            assert same_state(p, twin) and same_state(pool, twin), what
            seen.add(kind)
            t += k
    assert len(seen) == len(names), seen
    assert not batched or len(installed) == len(lists), installed
    assert not covariance or len(arrays) == len(ARRAY_LISTS), arrays


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m", [125, 1000])
@pytest.mark.parametrize("combo,opts", BOUNDED)
def test_analysis_entry_points_interleaved_on_one_plan(combo, opts, m, seed):
    """12 000 samples in 25 to 40 calls, each to one of sdft, sdft_every, power, power_sum, filterbank with a drawn grid, host and
    device memory in turn.  A twin plan takes the same cuts through sdft alone; a call's output is what numpy derives from the
    twin's rows of that call -- the rows on the grid, re * re + im * im of them -- and for the two calls that add (their order of
    addition is the library's) the library's own value from a plan that has seen none of the other entry points.  A filterbank
    row's bits depend on the plan, the filterbank and the row's powers alone: a third plan gives them for that call alone from the
    twin's state before it (sdft_hip_set_state).  A pooled row's bits depend on where the time chunks cut its window, and an
    installed state moves the chunks (its fid does not count as canonical, so the relay form, whose chunks begin on its block
    boundaries, is not taken): there the other plan follows the stream through sdft and makes only the pooled calls itself, with
    the same kind of memory; every == 1, first == 0 is numpy's powers as well.  After every call the plan's state is the twin's."""
    run_interleaved(combo, opts, m, seed)


# ---------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------
def test_filterbank_errors_leave_state_and_filterbank_untouched():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    sz = np.uint64
    with make(m, "hann", combo) as p:
        api = p.api
        out = np.zeros((10, m), dtype=np.float32)
        # no filterbank installed
        api.clear()
        assert p.filterbank_bands == 0
        assert api.sdft_filterbank_n(p._p, 100, x.ctypes.data, 10, 0, out.ctypes.data) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_filterbank_n" in err and "filterbank" in err, err
        api.clear()
        with pytest.raises(ValueError):
            p.filterbank(x[:10])
        bank = in_fd(random_bands(m), np.float32)
        p.set_filterbank(*bank)
        nbands = bank[0].size
        assert p.filterbank_bands == nbands
        p.filterbank(x[:300])                                 # (errors against a plan that is mid-stream)
        before = p.state()
        with make(m, "hann", combo) as q:                     # what the installed filterbank gives from here on
            q.set_filterbank(*bank)
            q.filterbank(x[:300])
            want = q.filterbank(x[300:900], 7, 2)

        def untouched(what):
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], what
            assert p.filterbank_bands == nbands, what

        big = np.zeros((10, nbands), dtype=np.float32)
        for n, every, ptr, word in [(100, 0, big.ctypes.data, "every"), (100, 10, None, "NULL")]:
            api.clear()
            assert api.sdft_filterbank_n(p._p, n, x.ctypes.data, every, 0, ptr) == -1, word
            err = api.last_error()
            assert err and "sdft_hip_sdft_filterbank_n" in err and word in err, err
            api.clear()
            untouched(word)
        w = np.ones(8, dtype=np.float32)
        refused = [(np.array([0, m - 3], dtype=sz), np.array([4, 4], dtype=sz), w.ctypes.data, "dftsize"),      # a band past dftsize
                   (np.array([0, m], dtype=sz), np.array([4, 1], dtype=sz), w.ctypes.data, "dftsize"),
                   (np.array([0, 2], dtype=sz), np.array([4, C.c_size_t(-1).value], dtype=sz), w.ctypes.data, "dftsize"),
                   (np.array([0, 9], dtype=sz), np.array([4, 0], dtype=sz), w.ctypes.data, "no bins"),          # a band of zero bins
                   (np.array([0, 9], dtype=sz), np.array([4, 4], dtype=sz), None, "NULL")]
        for b0, nb, wp, word in refused:
            api.clear()
            assert api.set_filterbank(p._p, 2, b0.ctypes.data, nb.ctypes.data, wp) == -1, word
            err = api.last_error()
            assert err and "sdft_hip_set_filterbank" in err and word in err, err
            api.clear()
            untouched(word)
        # n == 0: no rows, nothing moves
        assert api.sdft_filterbank_n(p._p, 0, x.ctypes.data, 10, 0, None) == 0 and api.last_error() is None
        untouched("n == 0")
        # the installed filterbank still answers as before
        assert np.array_equal(p.filterbank(x[300:900], 7, 2), want)
        # first >= n: no rows, out may be NULL, the state advances
        assert p.filterbank(x[900:1300], 10, 400).shape == (0, nbands)
        # no bands: the filterbank is removed
        p.set_filterbank([], [], [])
        assert p.filterbank_bands == 0
        api.clear()
        assert api.sdft_filterbank_n(p._p, 100, x.ctypes.data, 10, 0, big.ctypes.data) == -1
        api.clear()


# ---------------------------------------------------------------------------------------------
# a plain C host and a C++ host
# ---------------------------------------------------------------------------------------------
def host_link(hip_library):
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    return ["-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]


@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_filterbank(tmp_path, hip_library, flags, combo):
    """tests/c/host_filterbank.c: a stream in calls of ragged lengths, each with the documented next first, and the error returns
    through sdft_hip_last_error; its rows against SDFT.filterbank of the whole signal in one call (FD float: bit for bit)"""
    import torch
    td, fd, _ = O.combo_types(combo)
    exe = tmp_path / "host_filterbank"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_filterbank.c"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, nbands = 1000, 6000, 7, 24
    x, pw = expected(combo, "hann", m, n)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(tmp_path / "x.raw"), str(tmp_path / "rows.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-FILTERBANK ok" in r.stdout
    got = np.fromfile(tmp_path / "rows.raw", dtype=fd).reshape(-1, nbands)
    # the host's filterbank (host_filterbank.c): overlapping bands, wider than a tile
    start = np.arange(nbands) * m // 32
    length = np.minimum(m // 8 + 7 * np.arange(nbands), m - start)
    w = np.concatenate([(1 + (b * 31 + np.arange(length[b]) * 7) % 13) / 16 - 0.25 for b in range(nbands)])
    bank = in_fd((start.astype(np.uint64), length.astype(np.uint64), w), fd)
    p64 = torch.from_numpy(np.array(on_grid(pw, every, 0))).cuda().double()
    R, T, L, sum_w = reference(bank, p64)
    check_rows(got, R, T, L, sum_w, fd, 0.0 if exact_combo(combo) else float(p64.max()), ("C host", combo))
    with make(m, "hann", combo) as p:
        p.set_filterbank(*bank)
        tiles, per = geometry(p)
        assert (pieces_of(bank, per) > 1).sum() > nbands // 2
        want = p.filterbank(x, every, 0)
    assert got.shape == want.shape
    if exact_combo(combo):
        assert same_bits(got, want)


@pytest.mark.parametrize("t,f,combo", [("float", "double", "f32f64"), ("double", "double", "f64f64"), ("float", "float", "f32f32")])
def test_cpp_facade_filterbank(tmp_path, hip_library, t, f, combo):
    """tests/cpp/host_filterbank.cpp: sdft::SDFT<T, F>::set_filterbank, filterbank_bands, filterbank and power_sum, for the type
    pairs of test_cpp_facade_host; the host checks a whole-row band against the row sums of power_sum within the contract's bar
    and a one-bin bank against its rows bit for bit (calls of one time chunk: the powers of both calls are the same bits)"""
    td = O.combo_types(combo)[0]
    exe = tmp_path / "host_filterbank_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", f"-DHOST_T={t}", f"-DHOST_F={f}", "-I", os.path.join(ROOT, "include", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_filterbank.cpp"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n = 1000, 441
    signal(n, td, 9).tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(tmp_path / "x.raw")], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0 and "CPP-FILTERBANK ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
