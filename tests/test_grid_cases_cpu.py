"""The case generator of the grid sweep (tests/grid_cases.py) without a GPU: the draw is deterministic, every case meets the
preconditions of the call it describes, the stratified seeds fill every (kind x type pair x stratum) cell, and the 40 committed
seeds reach the geometries, grids and cuts the sweep exists for -- each at least three times, by the generator alone.  The same
for the second slate (cases2: the six newer calls), whose addition did not move a draw of the first."""

import hashlib

import numpy as np
import pytest

import grid_cases as G
from oracle import oracle as O

SEEDS = range(40)


@pytest.fixture(scope="module")
def drawn():
    return [c for s in SEEDS for c in G.cases(s, offset=0)]     # (the committed seeds, whatever campaign the environment names)


def test_the_draw_is_deterministic():
    assert G.COMBOS == O.COMBOS
    for s in (0, 13, 27, 39):
        a, b = G.cases(s, offset=0), G.cases(s, offset=0)
        assert repr(a) == repr(b) and len(a) == 7
        assert [c["slot"] for c in a] == list(G.SLOTS)
        assert all(c["kind"] == c["slot"] for c in a[:6]) and a[6]["kind"] in G.KINDS and a[6]["channels"] > 1
    assert repr(G.cases(3)) != repr(G.cases(4)) and repr(G.cases(3, offset=0)) != repr(G.cases(3, offset=1000))


def test_every_case_meets_the_preconditions_of_its_call(drawn):
    assert len(drawn) == 7 * len(SEEDS)
    for c in drawn:
        m, ch, n1, o = c["m"], c["channels"], c["n1"], c["opts"]
        assert c["combo"] == G.COMBOS[c["seed"] % 4] and c["window"] in G.WINDOWS, c
        assert m >= 1 and n1 >= 1 and c["n0"] >= 0 and c["every"] >= 1 and c["first"] >= 0, c
        assert m * n1 * ch <= G.BUDGET and (ch == 1 or (2 <= ch <= 5 and m <= 600)), c
        assert c["per"] == G.geometry(c["combo"], c["window"], o.get("interior", 0))[2] and c["tiles"] == -(-m // c["per"]), c
        # only the keys the sweep lists, the hooks' keys on hooks plans only
        assert set(o) <= {"chunk", "carry", "segments", "chain", "float_carry_parallel", "stage_bytes", "interior", "fft_carry", "fused", "prefix_cells"}, c
        assert c["hooks"] or not set(o) & {"interior", "fft_carry", "fused", "prefix_cells"}, c
        assert o.get("chunk", 0) in G.CHUNKS + (128, 256) and o.get("segments", 0) in (0, 1, 2, 3, 5) and o.get("chain", 1) in (0, 1, 2), c
        assert o.get("interior", 8) in (8, 24, 62) and o.get("fft_carry", 0) in (0, 1, 2) and o.get("prefix_cells", 0) in (0, 2), c
        assert "stage_bytes" not in o or (not c["device"] and G.exact_mode(c)), c
        assert c["out"] is None or c["device"], c
        assert c["warm"] in ("sdft", "every", "power", "power_sum", c["kind"]), c
        for band in [c["warm_band"]] + ([c["band"]] if c["kind"] in G.BANDED else []):
            assert 0 <= band[0] and band[1] >= 1 and band[0] + band[1] <= m, c
        assert ("band" in c) == (c["kind"] in G.BANDED), c
        if c["kind"] == "every":
            assert (c["every"], c["first"]) != (1, 0), c
        if c["kind"] == "filterbank":
            assert all(b0 >= 0 and nb >= 1 and b0 + nb <= m for b0, nb in c["bank"]["extra"]), c
        if c["kind"] == "cross_sum":
            assert c["pairs"] and all(0 <= a < ch and 0 <= b < ch for a, b in c["pairs"]), c
        if c["kind"] == "covariance":
            assert c["array"] and len(set(c["array"])) == len(c["array"]) and all(0 <= a < ch for a in c["array"]), c
        assert not c["fid_scale"] or (c["stratum"] == "installed" and ch > 1), c


def test_every_stratum_is_what_its_name_claims(drawn):
    """the pins of the strata, from the restated route logic: what the GPU test then asserts of the library's own answers"""
    for c in drawn:
        o, m, n1, s = c["opts"], c["m"], c["n1"], c["stratum"]
        exact, cuts = G.exact_mode(c), G.chunk_cuts(c)
        assert s == (G.STRATA[(c["seed"] // 4) % 7] if c["seed"] < G.STRATIFIED else "free"), c
        if s == "default":
            assert not set(o) & {"chunk", "carry", "segments", "chain", "float_carry_parallel"}, c
        if s == "one_chunk":
            assert n1 < G.HOP and cuts == [(0, n1)], c
        if s in ("relay", "serial", "sums", "segments", "installed"):
            assert n1 >= G.HOP or (cuts is not None and len(cuts) > 1), c
            assert exact == (s != "sums"), c
        if s == "relay":
            length = G.chunk_len_of(c) or 128               # (the library's own choice on exact carries: whole blocks of 128)
            block = G.relay_block(m, length, c["combo"], o.get("chain", 1), c["channels"])
            assert block and c["n0"] % block and o.get("chain", 1) != 0, c
        if s == "serial":
            assert o.get("chain", 1) == 0 or not any((2 * m) % b == 0 for b in (8, 16, 32, 64, 128)), c
        if s == "sums":
            assert ("float_carry_parallel" in o) == (not G.fd_double(c["combo"])) and o.get("carry", 0) == 0, c
        if s == "segments":
            assert o["segments"] == 3 and len(cuts) >= 3, c
        if s == "installed" and cuts is not None:
            assert all(t0 == j * (cuts[0][1] - cuts[0][0]) for j, (t0, _) in enumerate(cuts)), c      # (no relay form: no shift)
    sums = [c for c in drawn if c["stratum"] == "sums"]
    for kind in G.KINDS:
        assert {G.smooth(2 * c["m"]) for c in sums if c["kind"] == kind} == {True, False}, kind


def test_the_stratified_seeds_fill_every_cell(drawn):
    cells = {(c["slot"], c["combo"], c["stratum"]) for c in drawn if c["seed"] < G.STRATIFIED}
    assert cells == {(k, combo, s) for k in G.SLOTS for combo in G.COMBOS for s in G.STRATA} and len(cells) == 7 * 4 * 7
    assert all(c["stratum"] == "free" for c in drawn if c["seed"] >= G.STRATIFIED)
    mixed = {c["kind"] for c in drawn if c["slot"] == "mixed"}
    assert len(mixed) >= 4, mixed


def test_the_committed_seeds_reach_what_the_sweep_is_for(drawn):
    count = dict.fromkeys(["last tile owns one bin", "last tile exactly full", "one bin just below a boundary", "one bin just above a boundary",
                           "two bins across a boundary", "power at every 8", "power at every 9", "first >= n1", "a window cut by three chunks",
                           "a chunk inside one window", "windows that are the chunks", "a chunk no multiple of 8 on exact carries",
                           "a cursor off every block length", "every beside the chunk length", "a band over three tiles", "a per-channel fid",
                           "a guarded output", "a staged host call", "a bank band that ends on a boundary", "a bank band that begins on one"], 0)

    def hit(name, yes=True):
        count[name] += bool(yes)

    for c in drawn:
        m, per, tiles, n1, every, first = c["m"], c["per"], c["tiles"], c["n1"], c["every"], c["first"]
        hit("last tile owns one bin", tiles >= 2 and m - (tiles - 1) * per == 1)
        hit("last tile exactly full", m % per == 0)
        if "band" in c:
            b0, nb = c["band"]
            inner = b0 % per == 0 and b0 > 0                              # b0 is a tile's own0, with a tile below it
            hit("one bin just above a boundary", nb == 1 and inner)
            hit("one bin just below a boundary", nb == 1 and (b0 + 1) % per == 0 and b0 + 1 < m)
            hit("two bins across a boundary", nb == 2 and (b0 + 1) % per == 0)
            hit("a band over three tiles", (b0 + nb - 1) // per - b0 // per >= 2)
        if c["kind"] == "power":
            hit("power at every 8", every == 8)
            hit("power at every 9", every == 9)
        hit("first >= n1", first >= n1)
        cuts = G.chunk_cuts(c)
        if c["kind"] in G.POOLED and cuts is not None and len(cuts) > 1:
            w = G.windows(n1, every, first)
            touched = [sum(1 for t0, t1 in cuts if t0 < e and b < t1) for b, e in w]
            hit("a window cut by three chunks", max(touched) >= 3)
            hit("a chunk inside one window", any(b < t0 and t1 < e for t0, t1 in cuts for b, e in w))
            hit("windows that are the chunks", w == cuts)
        hit("a chunk no multiple of 8 on exact carries", G.exact_mode(c) and c["opts"].get("chunk", 0) % 8 != 0)
        hit("a cursor off every block length", (c["n0"] % (2 * m)) % 8 != 0)
        L = G.chunk_len_of(c)
        hit("every beside the chunk length", cuts is not None and len(cuts) > 1 and every in (L - 1, L, L + 1))
        hit("a per-channel fid", c["fid_scale"])
        hit("a guarded output", c["out"] is not None)
        hit("a staged host call", "stage_bytes" in c["opts"])
        if c["kind"] == "filterbank":
            hit("a bank band that ends on a boundary", any((b0 + nb) % per == 0 and b0 + nb < m for b0, nb in c["bank"]["extra"]))
            hit("a bank band that begins on one", any(b0 % per == 0 and b0 > 0 for b0, nb in c["bank"]["extra"]))
    print(count)
    short = {k: v for k, v in count.items() if v < 3}
    assert not short, (short, count)


# ---------------------------------------------------------------------------------------------
# the second slate: mix, power_peak, lag_sum, power_moments, band_peak, power_smooth
# ---------------------------------------------------------------------------------------------
def test_the_first_slate_did_not_move():
    """the digest of the first slate's 280 cases as they were drawn before the second slate existed"""
    h = hashlib.sha256()
    for s in SEEDS:
        h.update(repr(G.cases(s, offset=0)).encode())
    assert h.hexdigest() == "b5640469cc23c6dc8c07ad35884fb921221b74496e6dfb67d2387ebe22b62476"


@pytest.fixture(scope="module")
def drawn2():
    return [c for s in SEEDS for c in G.cases2(s, offset=0)]


def several_chunks(c):
    cuts = G.chunk_cuts(c)
    return c["n1"] >= G.HOP or (cuts is not None and len(cuts) > 1)


def test_the_second_draw_is_deterministic():
    assert G.BASE2 != G.BASE and abs(G.BASE2 - G.BASE) > 2000      # (no seed or campaign offset of one slate is a seed of the other)
    assert G.SLOTS2 == G.KINDS2 + ("mixed",) and not set(G.KINDS) & set(G.KINDS2)
    assert [G.KERNEL[k] for k in G.KINDS + G.KINDS2] == list(range(4, 16))
    for s in (0, 13, 27, 39):
        a, b = G.cases2(s, offset=0), G.cases2(s, offset=0)
        assert repr(a) == repr(b) and len(a) == 7
        assert [c["slot"] for c in a] == list(G.SLOTS2)
        assert all(c["kind"] == c["slot"] for c in a[:6]) and a[6]["kind"] in G.KINDS2 and a[6]["channels"] > 1
    assert repr(G.cases2(3)) != repr(G.cases2(4)) and repr(G.cases2(3, offset=0)) != repr(G.cases2(3, offset=1000))


def test_every_case_of_the_second_slate_meets_the_preconditions_of_its_call(drawn2):
    from sdft_amd.sdft import every_next_first, smooth_coefficients, smooth_decay
    assert len(drawn2) == 7 * len(SEEDS)
    for c in drawn2:
        m, ch, n1, o, kind = c["m"], c["channels"], c["n1"], c["opts"], c["kind"]
        fd = np.float64 if G.fd_double(c["combo"]) else np.float32
        assert c["combo"] == G.COMBOS[c["seed"] % 4] and c["window"] in G.WINDOWS and kind in G.KINDS2, c
        assert m >= 1 and n1 >= 1 and c["n0"] >= 0 and c["every"] >= 1 and c["first"] >= 0, c
        assert m * n1 * ch <= G.BUDGET and (ch == 1 or (2 <= ch <= 5 and m <= 600)), c
        assert c["per"] == G.geometry(c["combo"], c["window"], o.get("interior", 0))[2] and c["tiles"] == -(-m // c["per"]), c
        assert set(o) <= {"chunk", "carry", "segments", "chain", "float_carry_parallel", "stage_bytes", "interior", "fft_carry", "fused", "prefix_cells"}, c
        assert c["hooks"] or not set(o) & {"interior", "fft_carry", "fused", "prefix_cells"}, c
        assert o.get("chunk", 0) in G.CHUNKS + (128, 256) and o.get("segments", 0) in (0, 1, 2, 3, 5) and o.get("chain", 1) in (0, 1, 2), c
        assert o.get("interior", 8) in (8, 24, 62) and o.get("fft_carry", 0) in (0, 1, 2) and o.get("prefix_cells", 0) in (0, 2), c
        assert "stage_bytes" not in o or (not c["device"] and G.exact_mode(c)), c
        assert c["out"] is None or c["device"], c
        if c["out"] is not None:                             # a residue the element size allows: 2 x for the complex outputs
            size = (8 if G.fd_double(c["combo"]) else 4) * (2 if kind in ("mix", "lag_sum") else 1)
            assert c["out"] == (16, 128) or (c["out"][1] == 16 and 0 < c["out"][0] < 16 and c["out"][0] % size == 0), c
        assert c["warm"] in ("sdft", "every", "power", "power_sum", kind), c
        for band in [c["warm_band"]] + ([c["band"]] if kind in G.BANDED else []):
            assert 0 <= band[0] and band[1] >= 1 and band[0] + band[1] <= m, c
        assert ("band" in c) == (kind in G.BANDED) == (kind != "band_peak"), c
        assert ("bank" in c) == (kind == "band_peak"), c
        # the split: a cut inside the call, never with host staging or a guarded output; its parts are the stream
        cut = c["split"]
        assert cut is None or (1 <= cut < n1 and "stage_bytes" not in o and c["out"] is None), c
        parts = G.parts(c)
        assert len(parts) == (1 if cut is None else 2) and sum(q["n1"] for q in parts) == n1 and parts[0]["n0"] == c["n0"], c
        if cut is not None:
            assert parts[1]["n0"] == c["n0"] + cut and parts[1]["first"] == every_next_first(cut, c["every"], c["first"]) >= 0, c
        if kind == "mix":
            chan = c["chan"]
            assert ch > 1 and chan and len(set(chan)) == len(chan) and all(0 <= a < ch for a in chan) and c["nout"] in G.MIX_NOUTS, c
            assert c["hooks"] or not {"mix_group", "mix_block"} & set(c), c
            assert c.get("mix_group", 2) in G.MIX_GROUPS and c.get("mix_block", 1) in G.MIX_BLOCKS, c
        if kind == "power_peak":
            assert c["hold"] in ("max", "min"), c
        if kind == "band_peak":
            b = c["bank"]
            assert all(b0 >= 0 and nb >= 1 and b0 + nb <= m for b0, nb in b["extra"]) and 1 <= b["keep"] <= 3 * m, c
            assert not b["one_bin"] or m * len(range(c["first"], n1, c["every"])) * ch <= G.ONE_BIN_WORK, c
        if kind == "power_smooth":
            a, b = smooth_coefficients(c["decay"], fd)       # (raises for a decay the call would refuse)
            assert 0 <= a < 1 and (c["decay"] in G.DECAYS or c["decay"] == smooth_decay(c["tau"])) and 2 <= c["tau"] <= 2000, c
            assert c["state"] in ("none", "host", "device"), c
        assert not c["fid_scale"] or (c["stratum"] == "installed" and ch > 1), c


def test_every_stratum_of_the_second_slate_is_what_its_name_claims(drawn2):
    """as for the first slate; of a split case the first call keeps what the stratum pins"""
    for whole in drawn2:
        c = G.parts(whole)[0]
        o, m, n1, s = c["opts"], c["m"], c["n1"], c["stratum"]
        exact, cuts = G.exact_mode(c), G.chunk_cuts(c)
        assert s == (G.STRATA[(c["seed"] // 4) % 7] if c["seed"] < G.STRATIFIED else "free"), c
        if s == "default":
            assert not set(o) & {"chunk", "carry", "segments", "chain", "float_carry_parallel"}, c
        if s == "one_chunk":
            assert n1 < G.HOP and cuts == [(0, n1)], c
            assert all(G.chunk_cuts(q) == [(0, q["n1"])] for q in G.parts(whole)), c
        if s in ("relay", "serial", "sums", "segments", "installed"):
            assert several_chunks(c), c
            assert exact == (s != "sums"), c
        if s == "relay":
            length = G.chunk_len_of(c) or 128               # (the library's own choice on exact carries: whole blocks of 128)
            block = G.relay_block(m, length, c["combo"], o.get("chain", 1), c["channels"])
            assert block and c["n0"] % block and o.get("chain", 1) != 0, c
        if s == "serial":
            assert o.get("chain", 1) == 0 or not any((2 * m) % b == 0 for b in (8, 16, 32, 64, 128)), c
        if s == "sums":
            assert ("float_carry_parallel" in o) == (not G.fd_double(c["combo"])) and o.get("carry", 0) == 0, c
        if s == "segments":
            assert o["segments"] == 3 and len(cuts) >= 3, c
        if s == "installed" and cuts is not None:
            assert all(t0 == j * (cuts[0][1] - cuts[0][0]) for j, (t0, _) in enumerate(cuts)), c      # (no relay form: no shift)
    sums = [c for c in drawn2 if c["stratum"] == "sums"]
    for kind in G.KINDS2:
        assert {G.smooth(2 * c["m"]) for c in sums if c["kind"] == kind} == {True, False}, kind


def test_the_stratified_seeds_of_the_second_slate_fill_every_cell(drawn2):
    cells = {(c["slot"], c["combo"], c["stratum"]) for c in drawn2 if c["seed"] < G.STRATIFIED}
    assert cells == {(k, combo, s) for k in G.SLOTS2 for combo in G.COMBOS for s in G.STRATA} and len(cells) == 7 * 4 * 7
    assert all(c["stratum"] == "free" for c in drawn2 if c["seed"] >= G.STRATIFIED)
    mixed = {c["kind"] for c in drawn2 if c["slot"] == "mixed"}
    assert len(mixed) >= 4, mixed


def test_the_committed_seeds_of_the_second_slate_reach_what_it_is_for(drawn2):
    names = ["a mix with a channel that only advances", "a mix with nout > 1", "hold max", "hold min",
             "lag_sum at (1, 0) with n0 > 0 and several chunks", "lag_sum with n0 == 0", "a lag_sum chunk that starts at cursor 0",
             "a lag_sum chunk that starts elsewhere", "a pooled window cut by three chunks", "a band_peak band that a tile boundary splits",
             "power_smooth with three or more chunks", "power_smooth with decay == 0", "state none", "state host", "state device",
             "a per-channel fid", "last tile owns one bin"]
    fids = ["a per-channel fid before lag_sum at a cursor that is not 0", "a per-channel fid before lag_sum at cursor 0 after a warm-up"]
    names += [f"a split {k}" for k in G.KINDS2] + [f"a guarded {k}" for k in G.KINDS2]
    count = dict.fromkeys(names + fids, 0)

    def hit(name, yes=True):
        count[name] += bool(yes)

    for c in drawn2:
        if c["kind"] == "lag_sum" and c["fid_scale"] and c["n0"]:
            hit(fids[bool(c["n0"] % (2 * c["m"]) == 0)])
        m, per, tiles, n1, every, first, kind = c["m"], c["per"], c["tiles"], c["n1"], c["every"], c["first"], c["kind"]
        one = G.parts(c)[0]                                  # (of a split case: its first call)
        cuts = G.chunk_cuts(one)
        hit("last tile owns one bin", tiles >= 2 and m - (tiles - 1) * per == 1)
        hit("a per-channel fid", c["fid_scale"])
        hit(f"a split {kind}", c["split"] is not None)
        hit(f"a guarded {kind}", c["out"] is not None)
        if kind == "mix":
            hit("a mix with a channel that only advances", len(c["chan"]) < c["channels"])
            hit("a mix with nout > 1", c["nout"] > 1)
        if kind == "power_peak":
            hit("hold " + c["hold"])
        if kind == "lag_sum":
            hit("lag_sum at (1, 0) with n0 > 0 and several chunks", (every, first) == (1, 0) and c["n0"] > 0 and several_chunks(one))
            hit("lag_sum with n0 == 0", c["n0"] == 0)
            if cuts is not None:
                starts = [(one["n0"] + t0) % (2 * m) for t0, _ in cuts]
                hit("a lag_sum chunk that starts at cursor 0", 0 in starts)
                hit("a lag_sum chunk that starts elsewhere", any(starts))
        if kind in G.POOLED and cuts is not None and len(cuts) > 1:
            w = G.windows(one["n1"], every, first)
            hit("a pooled window cut by three chunks", max(sum(1 for t0, t1 in cuts if t0 < e and b < t1) for b, e in w) >= 3)
        if kind == "band_peak":
            fixed = [b for b in ((61, 2), (60, 4), (123, 2), (120, 8), (61, 63)) if b[0] + b[1] <= m]      # random_bands' own straddlers
            bands = [(0, m)] + fixed + [tuple(b) for b in c["bank"]["extra"]]
            hit("a band_peak band that a tile boundary splits", not c["bank"]["one_bin"] and any(b0 // per != (b0 + nb - 1) // per for b0, nb in bands))
        if kind == "power_smooth":
            hit("power_smooth with three or more chunks", cuts is not None and len(cuts) >= 3)
            hit("power_smooth with decay == 0", c["decay"] == 0)
            hit("state " + c["state"])
    print(count)
    # (only the two stratified seeds with a fid per channel can hold these: which form of the state the lag products' previous row takes)
    short = {k: v for k, v in count.items() if v < (1 if k in fids else 3)}
    assert not short, (short, count)
