"""The cases of the seeded sweep over the twelve grid analysis calls (tests/test_gpu_fuzz_grid.py), in two slates of six.  TEST
HELPER (plain numpy: no HIP, no torch; imported like guarded and exact_sdft).

cases(seed) draws the seven cases of a seed, one per kind in the order of SLOTS: the six grid entry points and `mixed`, a second
draw of one of the six on a batched plan.  The draw is deterministic: np.random.default_rng(BASE + seed + SDFT_FUZZ_OFFSET), the
environment variable tests/test_gpu_fuzz.py reads (a campaign beyond the committed seeds: SDFT_FUZZ_OFFSET=1000 pytest ...).

Seed s has the type pair COMBOS[s % 4]; the seeds 0 ... 27 have the stratum STRATA[(s // 4) % 7], so they fill every
(kind x type pair x stratum) cell; the seeds from 28 on are free draws (stratum "free").  A stratum pins the carry form of the
call under test, which the GPU test asserts:

    default    no route option                                                        the kernel only
    one_chunk  fewer than 512 samples, no chunk shorter than the call                 last_chunks == 1
    relay      exact carries, a block length dividing 2 m, chunks of whole blocks,    last_chain == 3, last_chunks > 1
               a warm-up that is no multiple of 8 samples (so chunk_shift != 0)
    serial     exact carries and chain = 0, or an m no block length divides 2 m of    last_chain == 0, last_chunks > 1
    sums       FD double carry = 0, FD float float_carry_parallel = 1; 2 m smooth     last_chain == 0, last_chunks > 1
               and not smooth in turn (the FFT forms and the direct partial sums)
    segments   exact carries, segments = 3, at least three chunks                     last_segments == 3
    installed  exact carries; the warm-up runs on a twin whose state is installed     last_chain == 0, last_chunks > 1
               (sdft_hip_set_state: the fid no longer counts as canonical); batched
               plans of every second pair of seeds get a fid of their own per channel

A case is a dict of plain values (its repr is the failure message of the GPU test, and all it takes to run the case again):
the plan (m, window, combo, channels, hooks, opts in the order they are set), the warm-up (n0 samples through the entry point
`warm`), the call under test (kind, n1 samples, every, first, band / bank / pairs / array), where the samples and the output
live (device, stage_bytes in opts, out = residue of a guarded output or None) and the seed of the samples.

The geometry is restated from logic::interior_lanes and logic::bins_per_lane (sdft_plan_logic.hpp); the GPU test asserts it
against the plan's own answers.  chunk_cuts() restates where a forced chunk length cuts time (logic::choose_grid_chunks,
logic::relay_block, logic::chunk_begin / chunk_end) for the coverage conditions of tests/test_grid_cases_cpu.py.

cases2(seed) is the second slate: the six newer calls (KINDS2: mix, power_peak, lag_sum, power_moments, band_peak, power_smooth) and
`mixed`, drawn from np.random.default_rng(BASE2 + seed + SDFT_FUZZ_OFFSET) by the same rule and through the same draws of the plan,
the options, the warm-up, the grid and the placement, so that a stratum means the same in both slates.  The first slate's draws
do not move: what a new kind draws, it draws on branches the old kinds never take (tests/test_grid_cases_cpu.py pins the digest).
A case of the second slate has, by kind: the mix (nout, chan, wseed: test_gpu_mix.weights_for(fdx, nout, len(chan), m, wseed);
mix_group / mix_block on hooks plans), hold, the smoothing (decay, tau where smooth_decay(tau) gave it, state in none / host /
device, sseed: test_gpu_power_smooth.some_state), the bank of band_peak (as the filterbank's; one_bin: one_bin_bands(m); keep: the
first `keep` of random_bands' 3 m bands), and split: None, or the sample at which the call under test is cut into two calls (in
the strata that pin several chunks the cut leaves them to the first call).  Where fid_scale is set, the second slate scales
channel c's fid by 2.0 ** c, which is exact in either FD type and passes through the demodulation and the window exactly."""

from __future__ import annotations

import os

import numpy as np

BASE = 52000
BASE2 = 137000                                               # the second slate's
OFFSET = int(os.environ.get("SDFT_FUZZ_OFFSET", "0"))
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")           # oracle.COMBOS (asserted by the tests)
WINDOWS = ("boxcar", "hann", "hamming", "blackman")
KINDS = ("every", "power", "power_sum", "filterbank", "cross_sum", "covariance")
SLOTS = KINDS + ("mixed",)
STRATA = ("default", "one_chunk", "relay", "serial", "sums", "segments", "installed")
STRATIFIED = 28                                              # seeds below this are stratified: 4 type pairs x 7 strata
KINDS2 = ("mix", "power_peak", "lag_sum", "power_moments", "band_peak", "power_smooth")
SLOTS2 = KINDS2 + ("mixed",)
KERNEL = {"every": 4, "power": 5, "power_sum": 6, "filterbank": 7, "cross_sum": 8, "covariance": 9,
          "mix": 10, "power_peak": 11, "lag_sum": 12, "power_moments": 13, "band_peak": 14, "power_smooth": 15}    # logic::ForwardKernel
POOLED = ("power_sum", "cross_sum", "covariance", "power_peak", "lag_sum", "power_moments")      # the kinds that pool windows (and have a head row)
BANDED = ("power", "power_sum", "cross_sum", "covariance", "mix", "power_peak", "lag_sum", "power_moments", "power_smooth")      # ... that take a band of bins
COMPLEX = ("every", "cross_sum", "covariance", "mix", "lag_sum")                                   # ... whose output elements are (re, im)

STRUCTURAL = (8, 9, 31, 63, 64, 65, 127, 128, 129, 500, 1000, 1023, 1024, 1025, 1100, 2047, 2048, 2049, 2500, 4096, 4100)   # tests/test_gpu_fuzz.py
CHUNKS = (0, 8, 64, 96, 100, 200, 512, 1000, 1 << 30)
BUDGET = 3_000_000                                           # m * n * channels of the call under test, as tests/test_gpu_fuzz.py
HOP = 512                                                    # logic::kHopSamples: shorter calls are one chunk unless option "chunk" cuts them
CLOSING = 60                                                 # samples of the closing sdft call
PAIR_WORK = 6_000_000                                        # pairs * n1 * band bins the reference of a pair case may cost
ONE_BIN_WORK = 2_000_000                                     # m * rows * channels up to which band_peak may get one_bin_bands(m)
BANK_BANDS = 600                                             # bands of random_bands(m) a band_peak case keeps (the reference is a loop over bands)
DECAYS = (0.0, 0.5, 0.9, 1.0 - 2.0 ** -10)                   # tests/test_gpu_power_smooth.py
MIX_NOUTS, MIX_GROUPS, MIX_BLOCKS = (1, 2, 3, 5), (2, 4, 8), (1, 2, 4)      # tests/test_gpu_mix.py

# the pair lists and arrays of the suites (the GPU test asserts that they are the suites' own)
PAIRS = [(0, 1), (1, 0), (2, 2), (0, 0), (0, 2), (0, 1)]     # tests/test_gpu_cross_sum.py
PAIR_LISTS = ([(3, 3)], [(2, 0), (1, 3)])                    # tests/test_gpu_filterbank.py
ARRAY_LISTS = ([3, 1, 0, 2], [2, 0], [1])


def seventy_pairs():
    """tests/test_gpu_cross_sum_routes.py seventy_pairs"""
    rng = np.random.default_rng(70)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 5, (70, 2))]
    pairs[10] = pairs[3]
    a, b = next(q for q in pairs if q[0] != q[1])
    pairs[20], pairs[40] = (a, b), (b, a)
    return pairs


WRITER_LISTS = {"a-only": [(0, 1), (2, 1)], "b-only-then-none": [(0, 1), (0, 2), (1, 2)], "auto-first": [(4, 4), (0, 4)],
                "seventy": seventy_pairs()}                  # tests/test_gpu_cross_sum_routes.py


# ---------------------------------------------------------------------------------------------
# the plan's geometry and the time chunks of a forced length, restated
# ---------------------------------------------------------------------------------------------
def fd_double(combo):
    return combo.endswith("f64")


def geometry(combo, window, forced=0):
    """(interior lanes, bins per lane, bins a tile owns) -- logic::interior_lanes, logic::bins_per_lane"""
    bpl = 1 if fd_double(combo) else 2
    halo = {"boxcar": 0, "blackman": 2}.get(window, 1)
    most = 64 - 2 * ((halo + bpl - 1) // bpl)
    interior = max(min(forced, most) if forced > 0 else (most // 8) * 8, 1)
    return interior, bpl, interior * bpl


def tiles_of(m, per):
    return (m + per - 1) // per


def exact_mode(case):
    """the plan's carries are the exact ones: FD float unless float_carry_parallel, FD double with carry = 1"""
    o = case["opts"]
    return (not o.get("float_carry_parallel")) if not fd_double(case["combo"]) else o.get("carry", 0) == 1


def relay_block(m, chunk_len, combo, chain=1, channels=1):
    """logic::relay_block behind logic::forward_route's chain_ok (fid canonical): the block length, 0 for the serial pass"""
    if chain == 0 or (chain < 2 and ((m + 31) // 32) * channels > 1024):
        return 0
    fdx = 16 if fd_double(combo) else 8
    for cand in (128, 64, 32, 16, 8):
        if cand > (64 if fd_double(combo) else 128):
            continue
        if (2 * m) % cand == 0 and chunk_len > 0 and chunk_len % cand == 0 and (2 * m // cand) * m * fdx <= (256 << 20):
            return cand
    return 0


def smooth(span):
    """logic::smooth_radices(span).count > 0: the FFT forms of the chunk partial sums exist"""
    for f in (2, 3, 5):
        while span % f == 0:
            span //= f
    return span == 1


def chunk_len_of(case):
    """the chunk length of the call under test where the case decides it (a forced chunk, a call of one chunk), else None"""
    chunk, n1 = case["opts"].get("chunk", 0), case["n1"]
    if chunk <= 0:
        return n1 if n1 < HOP else None
    return max(1, min(chunk if exact_mode(case) else (chunk + 7) // 8 * 8, n1))


def chunk_cuts(case):
    """[(t0, t1)] of the call's time chunks where the case decides them, else None (logic::chunk_begin, logic::chunk_end)"""
    n1, length = case["n1"], chunk_len_of(case)
    if length is None or case["opts"].get("stage_bytes"):
        return None
    shift = 0
    if exact_mode(case) and case["stratum"] != "installed" and length < n1:
        block = relay_block(case["m"], length, case["combo"], case["opts"].get("chain", 1), case["channels"])
        shift = (case["n0"] % (2 * case["m"])) % block if block else 0
    cuts, j = [], 0
    while (j * length - shift if j else 0) < n1:
        cuts.append((j * length - shift if j else 0, min((j + 1) * length - shift, n1)))
        j += 1
    return cuts


def windows(n, every, first):
    """[begin, end) of every row of a pooled call (tests/test_gpu_power_sum.py windows)"""
    w = [(0, min(first, n))] if first > 0 and n > 0 else []
    return w + [(b, min(b + every, n)) for b in range(first, n, every)]


# ---------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------
def pick(rng, seq):
    seq = list(seq)
    return seq[int(rng.integers(0, len(seq)))]


def maybe(rng, opts, key, values, p=0.5):
    if rng.random() < p:
        opts[key] = int(pick(rng, values))


def draw_opts(rng, stratum, combo, m, hooks, interior):
    """the options in the order they are set, and whether the stratum wants several chunks"""
    o = {}
    if hooks:
        if interior:
            o["interior"] = interior
        maybe(rng, o, "fft_carry", (0, 1, 2))
        maybe(rng, o, "fused", (0, 1), 0.3)
        maybe(rng, o, "prefix_cells", (0, 2), 0.3)
    dbl = fd_double(combo)
    if stratum == "one_chunk":
        maybe(rng, o, "chunk", (0, 512, 1000, 1 << 30))
        maybe(rng, o, "carry", (0, 1))
        maybe(rng, o, "segments", (0, 1, 2, 5))
        maybe(rng, o, "chain", (0, 1, 2))
    elif stratum == "relay":
        o["carry"] = 1 if dbl else int(rng.integers(0, 2))
        maybe(rng, o, "chunk", (0, 128, 256, 512), 0.7)
        maybe(rng, o, "chain", (1, 2))
        maybe(rng, o, "segments", (0, 1, 2, 5))
    elif stratum == "serial":
        if dbl or rng.random() < 0.5:
            o["carry"] = 1
        if m % 4 == 0:
            o["chain"] = 0
        else:
            maybe(rng, o, "chain", (0, 1, 2))
        maybe(rng, o, "chunk", (0, 8, 64, 96, 100, 200, 512, 1000), 0.7)
        maybe(rng, o, "segments", (0, 1, 2, 5))
    elif stratum == "sums":
        if dbl:
            maybe(rng, o, "carry", (0,))
        else:
            o["float_carry_parallel"] = 1
        maybe(rng, o, "chunk", (0, 8, 64, 96, 100, 200, 512, 1000), 0.7)
    elif stratum == "segments":
        if dbl or rng.random() < 0.5:
            o["carry"] = 1
        o["segments"] = 3
        o["chunk"] = int(pick(rng, (64, 96, 100, 128, 200)))
        maybe(rng, o, "chain", (0, 1, 2))
    elif stratum == "installed":
        if dbl or rng.random() < 0.5:
            o["carry"] = 1
        maybe(rng, o, "chunk", (0, 8, 64, 96, 100, 200, 512, 1000), 0.7)
        maybe(rng, o, "chain", (1, 2))
        maybe(rng, o, "segments", (0, 1, 2, 5))
    elif stratum == "free":
        maybe(rng, o, "chunk", CHUNKS, 0.7)
        maybe(rng, o, "carry", (0, 1))
        maybe(rng, o, "segments", (0, 1, 2, 5))
        maybe(rng, o, "chain", (0, 1, 2))
    return o


def draw_m(rng, stratum, per, batched, alternate):
    geo = [1, 2, 3, 5, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per + 1]
    pool = [v for v in (geo if rng.random() < 0.6 else STRUCTURAL) if v >= 1 and (not batched or v <= 600)]
    if stratum == "relay":                                   # a block of 8 ... divides 2 m
        pool = [v for v in pool if v % 4 == 0] or [v for v in STRUCTURAL if v % 4 == 0 and (not batched or v <= 600)]
    if stratum == "sums":                                    # 2 m smooth and not smooth in turn
        pool = [v for v in pool if smooth(2 * v) == alternate] or [v for v in STRUCTURAL if smooth(2 * v) == alternate and (not batched or v <= 600)]
    return int(pick(rng, pool))


def draw_band(rng, m, per):
    """a band placed from the plan's real tiles; falls back to a drawn band where the plan has too few tiles for the kind"""
    tiles = tiles_of(m, per)
    mid = tiles // 2                                         # a tile with a lower neighbour wherever the plan has two tiles
    kind = int(rng.integers(0, 9))
    band = None
    if kind == 0:
        band = (0, m)
    elif kind == 1:
        band = (0, 1)
    elif kind == 2:
        band = (m - 1, 1)
    elif kind == 3 and tiles >= 2:
        band = (mid * per, 1)                                # the tile's own0: just above a boundary
    elif kind == 4 and tiles >= 2:
        band = (mid * per - 1, 1)                            # the lower tile's own1 - 1: just below it
    elif kind == 5 and tiles >= 2:
        band = (mid * per - 1, 2)                            # one bin on either side
    elif kind == 6 and m >= 2:
        b0 = 1 + 2 * int(rng.integers(0, m // 2))            # odd start, odd length: the FD float pair store
        band = (b0, 1 + 2 * int(rng.integers(0, (m - b0 + 1) // 2)))
    elif kind == 7 and tiles >= 3:
        t = int(rng.integers(0, tiles - 2))
        b0 = t * per + int(rng.integers(0, per))
        b1 = max((t + 2) * per + 1, int(rng.integers(b0 + 1, m + 1)))
        band = (b0, min(b1, m) - b0)
    if band is None:
        b0 = int(rng.integers(0, m))
        band = (b0, int(rng.integers(1, m - b0 + 1)))
    assert 0 <= band[0] and band[1] >= 1 and band[0] + band[1] <= m, (band, m, per)
    return band


def cut_to(pairs, channels):
    return [(a, b) for a, b in pairs if a < channels and b < channels] or [(0, 0)]


def draw_kind2(rng, case, several, length):
    """what only a kind of the second slate draws"""
    kind, ch, n1, stratum = case["kind"], case["channels"], case["n1"], case["stratum"]
    if kind == "mix":
        case["nout"] = int(pick(rng, MIX_NOUTS))
        form = int(rng.integers(0, 3))
        if form == 0:
            chan = list(range(ch))                           # all channels, in plan order
        elif form == 1:
            chan = [int(c) for c in rng.permutation(ch)[:int(rng.integers(1, ch))]]      # a proper subset: some channel only advances
            if len(chan) > 1 and chan == sorted(chan):
                chan.reverse()
        else:
            chan = [int(rng.integers(0, ch))]
        case["chan"], case["wseed"] = chan, int(rng.integers(0, 1 << 16))
        if case["hooks"]:
            maybe(rng, case, "mix_group", MIX_GROUPS, 0.3)
            maybe(rng, case, "mix_block", MIX_BLOCKS, 0.3)
    if kind == "power_peak":
        case["hold"] = str(pick(rng, ("max", "min")))
    if kind == "power_smooth":
        case["tau"] = float(rng.uniform(2.0, 2000.0))
        case["decay"] = float(pick(rng, DECAYS + (float(np.exp(-1.0 / case["tau"])),)))      # (smooth_decay(tau))
        case["state"] = str(pick(rng, ("none", "host", "device")))
        case["sseed"] = int(rng.integers(0, 1 << 16))
    # the call under test as two calls: the first keeps what the stratum pins
    low = (3 * length + 1) if stratum == "segments" else ((length + 1) if case["opts"].get("chunk", 0) > 0 else HOP) if several else 1
    take = rng.random() < 0.25
    case["split"] = None
    if take and n1 >= 2 and low < n1 and "stage_bytes" not in case["opts"] and case["out"] is None:
        case["split"] = int(rng.integers(low, n1))


def next_first(n, every, first):
    """sdft_amd.sdft.every_next_first"""
    rows = (n - first + every - 1) // every if first < n else 0
    return first + rows * every - n if rows else first - n


def parts(case):
    """the calls the call under test is made as: [case] or, for a split case, the two cases of its parts"""
    cut = case.get("split")
    if not cut:
        return [case]
    a = dict(case, n1=cut, split=None)
    b = dict(case, n0=case["n0"] + cut, n1=case["n1"] - cut, first=next_first(cut, case["every"], case["first"]), split=None)
    return [a, b]


def draw_case(rng, seed, slot, kind, combo, stratum, index):
    batched = slot == "mixed" or kind in ("cross_sum", "covariance", "mix") or (kind == "lag_sum" and stratum == "installed") or rng.random() < 1 / 3
    channels = int(rng.integers(2, 6)) if batched else 1
    window = WINDOWS[int(rng.integers(0, 4))]
    hooks = bool(rng.random() < 0.4)
    interior = int(pick(rng, (0, 8, 24, 62))) if hooks else 0
    lanes, bpl, per = geometry(combo, window, interior)
    m = draw_m(rng, stratum, per, batched, index % 2 == 0)
    opts = draw_opts(rng, stratum, combo, m, hooks, interior)
    case = dict(seed=seed, slot=slot, kind=kind, stratum=stratum, combo=combo, window=window, m=m, channels=channels, hooks=hooks,
                per=per, tiles=tiles_of(m, per), opts=opts)
    exact = exact_mode(case)

    # the call's length: within the budget; several chunks where the stratum wants them
    most = max(1, min(6000, BUDGET // (m * channels)))
    several = stratum in ("relay", "serial", "sums", "segments", "installed")
    if several and 0 < opts.get("chunk", 0) and (opts["chunk"] + 7) // 8 * 8 * (3 if stratum == "segments" else 1) >= most:
        opts["chunk"] = 64                                   # (a chunk the budget leaves no second one of)
    chunk = opts.get("chunk", 0)
    length = chunk if exact else (chunk + 7) // 8 * 8
    if stratum == "one_chunk":
        n1 = int(pick(rng, (1, 7, 8, 9, 511, int(rng.integers(1, HOP)), int(rng.integers(1, HOP)))))
        n1 = min(n1, most)
    elif stratum == "segments":
        n1 = int(rng.integers(3 * length + 1, most + 1))
    elif several:
        n1 = int(rng.integers((length + 1) if chunk > 0 else HOP, most + 1))
    else:
        n1 = int(pick(rng, (1, 9, 511, 512, 513))) if rng.random() < 0.25 else int(rng.integers(1, most + 1))
        n1 = min(n1, most)
    case["n1"] = n1

    # the warm-up: a call of n0 samples through a drawn entry point; it moves the cursor, and with it chunk_shift
    room = max(1, BUDGET // (m * channels))
    n0s = [0, 700, 2 * m - 1, 2 * m, 2 * m + 1, 128 * int(rng.integers(1, 6)), int(rng.integers(1, 701)), int(rng.integers(1, 701))]
    n0s = [v for v in n0s if 0 <= v <= room] or [0]
    if stratum == "relay":
        n0s = [v for v in n0s if v % 8] or [min(room, 2 * m - 1) | 1]
    case["n0"] = int(pick(rng, n0s))
    if kind == "lag_sum" and stratum not in ("relay", "installed") and rng.random() < 0.15:
        case["n0"] = 0                                       # (the zero previous row)
    case["warm"] = str(pick(rng, ("sdft", "every", "power", "power_sum", kind)))
    if stratum == "relay":
        assert case["n0"] % 8 and m % 4 == 0

    # the grid
    L = chunk_len_of(case) if 0 < chunk < (1 << 30) else None
    everys = [1, 2, 7, 8, 9, 100, n1 - 1, n1, n1 + 5, int(rng.integers(1, 601))] + ([L - 1, L, L + 1, 2 * L] if L else [])
    if kind == "power" and rng.random() < 0.35:
        everys = [8, 9]                                      # the last burst of the dense path, the first sparse grid
    if L and kind in POOLED and rng.random() < 0.3:
        everys = [L, 2 * L]
    every = int(pick(rng, [v for v in everys if v >= 1]))
    firsts = [0, every - 1, every, every + 1, int(rng.integers(0, every + 2)), int(rng.integers(0, every + 2))]
    first = int(pick(rng, [v for v in firsts if v >= 0]))
    if L and kind in POOLED and every == L and rng.random() < 0.5:
        first = 0                                            # windows that coincide with the chunks
    if rng.random() < 0.05:
        first = n1 + int(rng.integers(0, 3))                 # no grid rows; a pooled call has its head row only
    if kind == "every" and (every, first) == (1, 0):
        first = 1                                            # (every == 1, first == 0 is sdft_n itself: tests/test_gpu_fuzz.py)
    if kind in ("lag_sum", "power_moments") and rng.random() < 0.3:
        every, first = 1, 0                                  # a row is its term: the bit-for-bit check
    case["every"], case["first"] = every, first

    # what the call reads its bins, bands and channels from
    nb = m
    if kind in BANDED:
        case["band"] = draw_band(rng, m, per)
        nb = case["band"][1]
    if kind in ("filterbank", "band_peak"):
        extra, t = [], tiles_of(m, per) // 2
        bank = int(rng.integers(0, 3 if kind == "filterbank" else 4))      # random_bands(m), plus a band ending on / beginning on a tile boundary
        if bank == 1 and t >= 1:
            b0 = int(rng.integers(0, t * per))
            extra = [(b0, t * per - b0)]
        if bank == 2 and t >= 1:
            extra = [(t * per, int(rng.integers(1, m - t * per + 1)))]
        case["bank"] = dict(seed=int(rng.integers(0, 1 << 16)), extra=extra)
        if kind == "band_peak":
            rows = (n1 - first + every - 1) // every if first < n1 else 0
            case["bank"].update(one_bin=bool(bank == 3 and m * rows * channels <= ONE_BIN_WORK), keep=min(3 * m, BANK_BANDS))
    if kind == "cross_sum":
        lists = [("PAIRS", PAIRS), ("PAIR_LISTS[0]", PAIR_LISTS[0]), ("PAIR_LISTS[1]", PAIR_LISTS[1])] + list(WRITER_LISTS.items())
        lists = [(name, cut_to(p, channels)) for name, p in lists]
        lists = [(name, p) for name, p in lists if len(p) * n1 * nb <= PAIR_WORK] or [("auto", [(0, 0)])]
        case["pairs_name"], case["pairs"] = pick(rng, lists)
    if kind == "covariance":
        arrays = [[c for c in a if c < channels] for a in ARRAY_LISTS] + [list(range(channels))]
        case["array"] = [int(c) for c in pick(rng, [a for a in arrays if a])]
    case["warm_band"] = draw_band(rng, m, per)

    # where the samples and the output live
    guarded = rng.random() < 1 / 3                           # one case in three: the output carved from a guarded device arena
    case["device"] = bool(guarded or rng.random() < 0.4)
    if not case["device"] and exact and stratum in ("default", "free") and rng.random() < 0.4:
        opts["stage_bytes"] = int(pick(rng, (700 * channels * (8 if combo.startswith("f64") else 4), 4096, 65536)))
    case["out"] = None
    if guarded:
        size = (8 if fd_double(combo) else 4) * (2 if kind in COMPLEX else 1)
        case["out"] = pick(rng, [(r, 16) for r in range(size, 16, size)] + [(16, 128)])
    if kind in KINDS2:
        draw_kind2(rng, case, several, length)
    case["fid_scale"] = bool(stratum == "installed" and channels > 1 and (seed // 2) % 2 == 1)
    case["xseed"] = int(rng.integers(0, 1 << 20))
    return case


def cases(seed, offset=None):
    """the seven cases of a seed, in the order of SLOTS (offset: in place of SDFT_FUZZ_OFFSET)"""
    seed, offset = int(seed), OFFSET if offset is None else int(offset)
    rng = np.random.default_rng(BASE + seed + offset)
    combo = COMBOS[seed % 4]
    stratum = STRATA[(seed // 4) % 7] if seed < STRATIFIED else "free"
    out = []
    for i, slot in enumerate(SLOTS):
        kind = KINDS[int(rng.integers(0, 6))] if slot == "mixed" else slot
        out.append(draw_case(rng, seed, slot, kind, combo, stratum, seed + i + offset // 1000))
    return out


def cases2(seed, offset=None):
    """the seven cases of a seed of the second slate, in the order of SLOTS2"""
    seed, offset = int(seed), OFFSET if offset is None else int(offset)
    rng = np.random.default_rng(BASE2 + seed + offset)
    combo = COMBOS[seed % 4]
    stratum = STRATA[(seed // 4) % 7] if seed < STRATIFIED else "free"
    out = []
    for i, slot in enumerate(SLOTS2):
        kind = KINDS2[int(rng.integers(0, 6))] if slot == "mixed" else slot
        out.append(draw_case(rng, seed, slot, kind, combo, stratum, seed + i + offset // 1000))
    return out
