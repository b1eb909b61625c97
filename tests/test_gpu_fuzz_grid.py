"""Seeded, stratified sweep of the twelve grid analysis calls over the sizes, grids, bands and routes nobody picked by hand, on a real
MI355X, in two slates: sdft_hip_sdft_every_n, _power_n, _power_sum_n, _filterbank_n, _cross_sum_n, _covariance_n
(test_random_grid_call_parity) and sdft_hip_sdft_mix_n, _power_peak_n, _lag_sum_n, _power_moments_n, _band_peak_n, _power_smooth_n
(test_random_grid_call_parity_2).  tests/grid_cases.py draws the cases (seven per seed and slate; its docstring describes the
strata); a campaign beyond the committed seeds is SDFT_FUZZ_OFFSET=1000 pytest tests/test_gpu_fuzz_grid.py -s, and a failure's
message is the whole case.

A case is a warm-up call of n0 samples through a drawn entry point (it moves the cursor, and with it chunk_shift), the call under
test on the next n1 samples, and a closing sdft of 60 samples.  Each channel's stream goes through the oracle, call by call;
what numpy derives from the oracle's rows of the call is the expectation, by the helpers and bars of the call's own suite:

    every        the rows on the grid                           test_gpu_every.check         bits, or 1e-11 of the largest bin
    power        power_of(rows) on the grid and the band        test_gpu_power.check         bits, or BAR
    power_sum    wide-precision window sums of those powers     test_gpu_power_sum.check     gamma_L, + L BAR pmax when inexact
    filterbank   reference(bank, powers)                        test_gpu_filterbank.check_rows
    cross_sum,   numpy's unfused terms, summed per window       test_gpu_cross_sum.check_pairs (at (1, 0) on exact routes: the
    covariance                                                                                terms' bits)

    mix            the header's expression on the rows          test_gpu_mix.check_mix       bits, or promise (4)'s bar
    power_peak     the windows' extremes of the powers          test_gpu_power_peak.check    bits, or BAR pmax
    lag_sum        the terms A conj(B) on consecutive rows,     test_gpu_lag_sum.check_terms (at (1, 0) on exact routes: bits),
                   B of the first the row before the call       check_sums (promise 3, + L BAR max|X|^2 when inexact)
    power_moments  wide sums of p and of fl(p p)                test_gpu_power_moments.check_pair; at (1, 0) on exact routes p's
                                                                and fl(p p)'s bits; [..., 0] the bits of power_sum on a twin plan
    band_peak      peaks_of(bank, powers on the grid)           test_gpu_band_peak.same_pairs on exact routes; elsewhere the same
                                                                on a twin plan's power(), and the value within BAR pmax max|w|
    power_smooth   the recursion on the powers: loop() where    test_gpu_power_smooth.same_bits / within_bound (+ BAR pmax when
                   the call is one chunk on an exact route,     inexact), rows and returned state; decay 0 on exact routes: the
                   wide() elsewhere                             powers' bits on any chunking

A case is exact where test_gpu_fuzz.py says a call is -- FD float without float_carry_parallel, carry = 1, or a call of one time
chunk -- for the warm-up AND the call under test: an inexact warm-up leaves a state off by rounding.  On exact pair cases every
(b, a) is the conjugate of its (a, b), auto-pairs have im == +0, and the covariance call has the bits of the cross-spectrum call
of a twin plan that is given the same chunk length (as test_covariance_wide_array does).

FD float with float_carry_parallel = 1 (the stratum `sums`) is the one route none of the grid suites states a bar for: its rows
differ from the float oracle's by float rounding, so the 1e-11 of FD double's fast carries cannot apply.  What the project
promises of that option is tests/test_gpu_parity.py test_float_plans_with_chunk_parallel_carries: within 1e-4 of the
double-precision reference, relative to the largest bin.  So there the oracle is the FD double one of the same TD (its rows rounded
to float once), the row bar is 1e-4 in place of 1e-11, and the inexact terms of the helpers -- all of them BAR = 2.1 x the row bar
times a scale -- are scaled by 1e-4 / 1e-11 through the scale arguments the helpers take; the state and the closing hop are held
to 1e-4 likewise.  Nothing else about the checks changes.  The scale enters each header's formula once, in place of its constant:
the second moment's bar is L delta (2 pmax + delta) with delta = 2.1e-4 pmax, not a product of scaled factors.  (The committed
seeds hold these bars.  A campaign found one case that misses one: SDFT_FUZZ_OFFSET=16000, seed 19 of the second slate, band_peak at
m = 4100, 721 samples into a fresh plan, one row at sample 169: 1.0854e-11 against 2.1e-4 pmax max|w| = 1.0838e-11.  pmax is the
largest power of the call's grid, here of one early row of a window that is still filling, while the option's 1e-4 is stated
against the largest bin of the whole call; the bar is left as the header has it.)

With a fid of its own per channel (stratum `installed`, batched plans of every second pair of seeds) the oracle cannot follow:
the rows are those a twin plan's sdft gives from the same installed state, as
test_cross_sum_after_a_state_with_a_fid_of_its_own_per_channel has it.  The first slate scales channel c's fid by 1 + c / 1024,
the second by 2.0 ** c: a power of two passes through the demodulation and the window exactly, so the row before the lag-product
call's first sample is known too -- the header's "acc where the cursor is 0 modulo 2 dftsize, acc conj(fid) elsewhere": the
oracle's last warm-up row, times 2.0 ** c where the installed cursor is not 0.

One case in four of the second slate makes the call under test as two calls cut at a drawn sample (the second takes
every_next_first, and the smoothed state where there is one); head rows are joined by each header's rule (added, or the hold's
np.maximum / np.minimum) and the joined rows are checked as one call's -- in bits wherever the header says a row does not depend
on the cut.  The stratum's carry form is asserted of the first of the two calls.

After every case: the state of all channels against a twin that ran sdft alone (bits on exact routes, 1e-10 otherwise), the
closing hop against the oracle (bits, 1e-11; with fast carries a forced chunk shorter than the hop cuts the hop too, and then it
is held to 1e-11), the kernel, the stratum's carry form, and a forced chunk length honoured.  One case
in three hands the call an output carved from a guarded arena at a drawn residue: no byte outside it is written, none inside left.
The smoothed call's state array lies inside a larger one whose other elements are found untouched."""

import collections
import math
import types

import numpy as np
import pytest

import grid_cases as GC
import guarded as G
import test_gpu_band_peak as BP
import test_gpu_cross_sum as XS
import test_gpu_cross_sum_routes as XR
import test_gpu_every as EV
import test_gpu_filterbank as FB
import test_gpu_lag_sum as LS
import test_gpu_mix as MX
import test_gpu_power as PW
import test_gpu_power_moments as PM
import test_gpu_power_peak as PK
import test_gpu_power_smooth as SM
import test_gpu_power_sum as PS
from oracle import oracle as O
from sdft_amd.sdft import SDFT, covariance_pairs, every_rows, power_sum_rows, smooth_decay

pytestmark = pytest.mark.gpu
LOOSE_ROW_BAR, ROW_BAR = 1e-4, EV.BAR                        # float_carry_parallel (tests/test_gpu_parity.py); FD double's fast carries
LOOSE = LOOSE_ROW_BAR / ROW_BAR                              # what the helpers' inexact scales are multiplied by on that route
assert ROW_BAR == 1e-11 and PW.BAR == 2.1 * ROW_BAR and MX.E_ROW == ROW_BAR and LS.BAR == PM.BAR == PK.BAR == SM.BAR == PW.BAR
assert GC.COMBOS == O.COMBOS and GC.PAIRS == XS.PAIRS and GC.PAIR_LISTS == FB.PAIR_LISTS and GC.ARRAY_LISTS == FB.ARRAY_LISTS
assert GC.WRITER_LISTS == XR.WRITER_LISTS and tuple(GC.WINDOWS) == tuple(PW.WINDOWS)
assert GC.DECAYS == SM.DECAYS and GC.MIX_NOUTS == tuple(MX.NOUTS) and (GC.MIX_GROUPS, GC.MIX_BLOCKS) == (MX.GROUPS, MX.BLOCKS)
assert GC.KERNEL["power_moments"] == PM.KERNEL
TALLY = collections.Counter()                                # (kind, stratum, last_chain, chunks) of the calls under test of this run
RAN = collections.Counter()                                  # the checks of the second slate that ran, by name
STATE_PAD, STATE_MARK = 24, -7.25                            # elements around the smoothed call's state array, and what they hold


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def new_plan(case, lists=True):
    p = SDFT(case["m"], case["window"], 1.0, case["combo"], case["channels"], hooks=case["hooks"])
    for k, v in case["opts"].items():
        p.set_option(k, v)
    if lists:
        install(p, case)
    return p


def bank_of(case, fd):
    """random_bands(m) as the filterbank suite draws them (the first `keep` of them where the case says so), plus the case's bands
    that end or begin on a tile boundary; or one_bin_bands(m)"""
    if case["bank"].get("one_bin"):
        return FB.in_fd(FB.one_bin_bands(case["m"]), fd)
    start, length, w = FB.random_bands(case["m"], 1000 + case["bank"]["seed"])
    keep = case["bank"].get("keep")
    if keep is not None and keep < start.size:
        start, length, w = start[:keep], length[:keep], w[:int(length[:keep].sum())]
    extra = case["bank"]["extra"]
    if extra:
        rng = np.random.default_rng(case["bank"]["seed"])
        start = np.concatenate([start, np.array([b for b, _ in extra], dtype=np.uint64)])
        length = np.concatenate([length, np.array([k for _, k in extra], dtype=np.uint64)])
        w = np.concatenate([w, rng.uniform(2.0 ** -10, 1.0, sum(k for _, k in extra))])
    return FB.in_fd((start, length, w), fd)


def weights_of(case, fdx):
    return MX.weights_for(fdx, case["nout"], len(case["chan"]), case["m"], case["wseed"])


def install(p, case):
    if case["kind"] in ("filterbank", "band_peak"):
        p.set_filterbank(*bank_of(case, p.fd))
    if case["kind"] == "cross_sum":
        p.set_pairs([a for a, _ in case["pairs"]], [b for _, b in case["pairs"]])
        assert p.pairs == len(case["pairs"])
    if case["kind"] == "covariance":
        p.set_array(case["array"])
        assert p.array_channels == len(case["array"])
    if case["kind"] == "mix":
        p.set_mix(weights_of(case, p.fdx), case["chan"])
        for key in ("mix_group", "mix_block"):
            if key in case:
                p.set_option(key, case[key])
                assert p.get_option(key) == case[key]
        assert p.mix_outputs == case["nout"]


def call(p, name, x, every, first, band, out=None, case=None, state=None):
    if name == "sdft":
        return p.sdft(x)
    if name == "every":
        return p.sdft_every(x, every, first, out=out)
    if name in ("filterbank", "band_peak"):
        return getattr(p, name)(x, every, first, out=out)
    if name == "lag_sum":
        return p.lag_sum(x, every, first, band=band, out=out)
    if name == "power_peak":
        return p.power_peak(x, every, first, bins=band, hold=case["hold"], out=out)
    if name == "power_smooth":
        return p.power_smooth(x, case["decay"], every, first, bins=band, state=state, out=out)
    return getattr(p, name)(x, every, first, bins=band, out=out)


def output_shape(case, p):
    n1, every, first, ch = case["n1"], case["every"], case["first"], case["channels"]
    kind = case["kind"]
    lead = (ch,) if ch > 1 else ()
    if kind == "every":
        return lead + (every_rows(n1, every, first), case["m"]), p.fdx
    if kind in ("power", "power_smooth"):
        return lead + (every_rows(n1, every, first), case["band"][1]), p.fd
    if kind in ("power_sum", "power_peak"):
        return lead + (power_sum_rows(n1, every, first), case["band"][1]), p.fd
    if kind == "filterbank":
        return lead + (every_rows(n1, every, first), p.filterbank_bands), p.fd
    if kind == "band_peak":
        return lead + (every_rows(n1, every, first), p.filterbank_bands, 2), p.fd
    if kind == "power_moments":
        return lead + (power_sum_rows(n1, every, first), case["band"][1], 2), p.fd
    if kind == "lag_sum":
        return lead + (power_sum_rows(n1, every, first), case["band"][1]), p.fdx
    if kind == "mix":
        return (case["nout"], every_rows(n1, every, first), case["band"][1]), p.fdx
    items = len(case["pairs"]) if kind == "cross_sum" else len(case["array"]) * (len(case["array"]) + 1) // 2
    return (items, power_sum_rows(n1, every, first), case["band"][1]), p.fdx


def wide_sums(pw, w):
    """the window sums of the powers pw (n, k) in the wide dtype of tests/test_gpu_power_sum.py (float64 for FD float; long double,
    and math.fsum for windows of 2048 samples and more, for FD double), and the windows' lengths"""
    hi = PS.wide(pw.dtype)
    out = np.empty((len(w), pw.shape[1]), dtype=hi)
    for r, (b, e) in enumerate(w):
        if e - b == 1:
            out[r] = pw[b]
        elif hi is np.float64 or e - b < 2048:
            out[r] = pw[b:e].astype(hi).sum(axis=0)
        else:
            out[r] = [math.fsum(pw[b:e, k]) for k in range(pw.shape[1])]
    return out, np.array([e - b for b, e in w])


def check_state(p, q, exact, bar, what):
    """all channels, whether or not a pair, an array or a mix names them"""
    a, b = p.state(), q.state()
    assert a[3] == b[3] and np.array_equal(a[2], b[2]), what
    for name, u, v in (("acc", a[0], b[0]), ("fid", a[1], b[1])):
        u, v = np.atleast_2d(u), np.atleast_2d(v)
        for c in range(u.shape[0]):
            if exact:
                assert XS.same_bits(u[c].copy(), v[c].copy()), (what, name, c)
            else:
                assert PW.rel(u[c], v[c]) <= bar, (what, name, c, PW.rel(u[c], v[c]))


def route_of(p):
    return {k: p.get_option("last_" + k) for k in ("kernel", "chunks", "chunk_len", "chain", "segments")}


def twin_plan(cx, lists, same_warm):
    """a plan of the case's kind and options in the state the plan under test had before the call under test: the installed state,
    or the warm-up samples through sdft -- through the warm-up's own entry point and memory where the route is not exact, so that
    the state is the same bits (the same plan, options and input give the same bits on every run)"""
    case = cx.case
    t = new_plan(case, lists=lists)
    if case["stratum"] == "installed":
        t.set_state(*cx.installed)
    elif case["n0"]:
        if same_warm:
            call(t, case["warm"], cx.x0in, 7, 3, tuple(case["warm_band"]), case=case)
        else:
            t.sdft(cx.x0)
    return t


def twin_parts(cx, name, what):
    """what the entry point `name` returns, part by part, on a twin plan from the same state that is given each part's chunk length;
    the twin cuts time as the call under test did"""
    outs = []
    with twin_plan(cx, lists=True, same_warm=True) as t:
        for part, xin, route in zip(cx.parts, cx.xins, cx.routes):
            t.set_option("chunk", route["chunk_len"])
            outs.append(numpy_of(call(t, name, xin, part["every"], part["first"], cx.band, case=cx.case)))
            assert (t.get_option("last_chunk_len"), t.get_option("last_chunks")) == (route["chunk_len"], route["chunks"]), (what, name, route_of(t), route)
    return outs


def joined(cx, outs, pooled, join=None):
    """the parts' outputs as (channels or items, rows, ...), the rows of the parts one after the other; a pooled kind's head row
    completes the row before it by `join`"""
    lead = cx.ch > 1 or cx.kind in ("cross_sum", "covariance", "mix")
    outs = [o if lead else o[None] for o in outs]
    rows = outs[0]
    for part, o in zip(cx.parts[1:], outs[1:]):
        if pooled and part["first"] > 0:
            rows = rows.copy()
            rows[:, -1] = join(rows[:, -1], o[:, 0])
            o = o[:, 1:]
        rows = np.concatenate([rows, o], axis=1)
    return rows


# ---------------------------------------------------------------------------------------------
# the values of the first slate
# ---------------------------------------------------------------------------------------------
def check_first(cx):
    import torch
    case, kind, X, what, exact, loose, scale, band = cx.case, cx.kind, cx.X, cx.what, cx.exact, cx.loose, cx.scale, cx.band
    ch, n1, every, first, fd, route = cx.ch, case["n1"], case["every"], case["first"], cx.fd, cx.routes[0]
    g = cx.g
    if kind == "every":
        for c in range(ch):
            want = X[c][first::every]
            if loose:
                assert g[c].shape == want.shape and EV.rel(g[c], want) <= LOOSE_ROW_BAR, (what, c, EV.rel(g[c], want))
            else:
                EV.check(g[c], want, exact, (what, c))
    elif kind in ("power", "power_sum", "filterbank"):
        for c in range(ch):
            pw = PW.power_of(X[c])
            if kind == "power":
                want = np.ascontiguousarray(PW.on_grid(pw, every, first, band))
                if loose:
                    assert g[c].shape == want.shape and PW.deviation(g[c], want) <= 2.1 * LOOSE_ROW_BAR, (what, c, PW.deviation(g[c], want))
                else:
                    PW.check(g[c], want, exact, (what, c))
            elif kind == "power_sum":
                cols = pw[:, band[0]:band[0] + band[1]]
                want, lens = wide_sums(cols, GC.windows(n1, every, first))
                PS.check(g[c], want, lens, exact, float(cols.max()) * scale, (what, c))
                if (every, first) == (1, 0) and not loose:       # windows of one sample: the power call's values
                    PW.check(g[c], np.ascontiguousarray(cols), exact, (what, c, "one-sample windows"))
            else:
                bank = bank_of(case, fd)
                p64 = torch.from_numpy(pw).cuda().double()
                R, T, L, sum_w = FB.reference(bank, p64)
                rows = p64[first::every]
                inexact = 0.0 if exact or rows.numel() == 0 else float(rows.max()) * scale
                FB.check_rows(np.ascontiguousarray(g[c]), R[first::every], T[first::every], L, sum_w, fd, inexact, (what, c))
                del p64, R, T
    else:
        if kind == "cross_sum":
            pairs = [tuple(q_) for q_ in case["pairs"]]
        else:
            a, b = covariance_pairs(len(case["array"]))
            pairs = [(case["array"][i], case["array"][j]) for i, j in zip(a.tolist(), b.tolist())]
        cache = {}
        if loose:                                        # (check_pairs' inexact term is L BAR amax[a] amax[b])
            s = slice(band[0], band[0] + band[1])
            cache["amax"] = [float(np.abs(X[c][:, s]).max()) * math.sqrt(LOOSE) for c in range(ch)]
        XS.check_pairs(g, X, pairs, n1, every, first, band, exact, what, cache=cache)
        if exact:
            place = {}
            for j, (a, b) in enumerate(pairs):
                if a != b and (b, a) in place:
                    ba = g[place[(b, a)]]
                    assert XS.same_bits(g[j].real, ba.real) and np.array_equal(g[j].imag, -ba.imag), (what, "conjugate", j, (a, b))
                if a == b:
                    assert XS.same_bits(g[j].imag, np.zeros_like(g[j].imag)), (what, "auto-pair", j)
                place.setdefault((a, b), j)
        if kind == "covariance" and cx.mode_exact and not cx.staged:
            # the cross-spectrum call of a twin plan from the same state, given the covariance call's chunk length: the same bits
            with twin_plan(cx, lists=False, same_warm=False) as t:
                t.set_pairs([a for a, _ in pairs], [b for _, b in pairs])
                t.set_option("chunk", route["chunk_len"])
                same = numpy_of(t.cross_sum(cx.xins[0], every, first, bins=band))
                assert (t.get_option("last_kernel"), t.get_option("last_chunk_len"), t.get_option("last_chunks")) == (8, route["chunk_len"], route["chunks"]), what
                assert XS.same_bits(g, same), (what, "covariance against cross_sum")


# ---------------------------------------------------------------------------------------------
# the values of the second slate
# ---------------------------------------------------------------------------------------------
def smooth_reference(cx, pw, c, fn):
    """fn = loop or wide on channel c's powers from the drawn incoming state: one recursion over the n1 samples where the parts pass
    the state along, one per part from zero where they do not (state "none") -> the pieces' results, concatenated"""
    case = cx.case
    s0 = None if cx.s0 is None else np.atleast_2d(cx.s0)[c]
    if cx.s0 is not None or len(cx.parts) == 1:
        return [fn(pw, case["decay"], s0)]
    cut = cx.parts[0]["n1"]
    return [fn(np.ascontiguousarray(pw[:cut]), case["decay"], None), fn(np.ascontiguousarray(pw[cut:]), case["decay"], None)]


def check_second(cx):
    case, kind, X, what, exact, scale, band = cx.case, cx.kind, cx.X, cx.what, cx.exact, cx.scale, cx.band
    ch, n1, every, first, fd, g = cx.ch, case["n1"], case["every"], case["first"], cx.fd, cx.g
    dense = (every, first) == (1, 0)
    s = slice(band[0], band[0] + band[1]) if band else slice(0, case["m"])
    how = "bits" if exact else "bar"
    RAN[f"{kind} {how}"] += 1
    RAN[f"{kind} {how}, two calls"] += len(cx.parts) == 2
    if kind == "mix":
        MX.check_mix(g, X, case["chan"], weights_of(case, cx.fdx), every, first, band, exact, what, scale)
        return
    twin = None
    if kind == "power_moments" and case["device"] and all(r["segments"] == 1 for r in cx.routes):
        twin = joined(cx, twin_parts(cx, "power_sum", what), True, np.add)          # promise (2)
    if kind == "band_peak" and not exact:
        twin = joined(cx, twin_parts(cx, "power", what), False)                      # promise (4): power() of all bins on the grid
    bank = bank_of(case, fd) if kind == "band_peak" else None
    for c in range(ch):
        pw = PW.power_of(X[c])
        cols = np.ascontiguousarray(pw[:, s])
        pmax = float(cols.max())
        if kind == "power_peak":
            PK.check(g[c], PK.held_rows(cols, n1, every, first, case["hold"]), exact, pmax * scale, (what, c))
        elif kind == "lag_sum":
            prev, skip = cx.prev[c], int(cx.prev[c] is None)
            if exact and dense:
                LS.check_terms(g[c], X[c], prev, band, (what, c), skip)
                RAN["lag_sum terms, bits" + (", zero row before" if skip else "")] += c == 0
            if case["fid_scale"] and prev is not None:
                RAN["lag_sum after a fid per channel, cursor " + ("elsewhere" if case["n0"] % (2 * case["m"]) else "0")] += c == 0
            LS.check_sums(g[c], X[c], prev, n1, every, first, band, exact, (what, c), scale)
        elif kind == "power_moments":
            w = GC.windows(n1, every, first)
            want1, lens = wide_sums(cols, w)
            want2, _ = wide_sums(PM.squares(cols), w)
            PM.usable(PM.squares(cols), (what, c))
            PM.check_pair(g[c], want1, want2, lens, exact, pmax, (what, c), scale)
            if exact and dense:                              # promise (3): p and fl(p p), bit for bit
                assert np.array_equal(g[c][..., 0], cols) and np.array_equal(g[c][..., 1], PM.squares(cols)), (what, c, "one-sample windows")
                RAN["power_moments one-sample windows, bits"] += c == 0
            if twin is not None:
                assert np.array_equal(g[c][..., 0], twin[c]), (what, c, "[..., 0] against power_sum")
                RAN["power_moments [..., 0] against power_sum, bits"] += c == 0
        elif kind == "band_peak":
            grid = np.ascontiguousarray(pw[first::every])
            want = BP.peaks_of(bank, grid)
            if exact:
                assert BP.same_pairs(g[c], want), (what, c)
            else:
                assert BP.same_pairs(g[c], BP.peaks_of(bank, np.ascontiguousarray(twin[c]))), (what, c, "the expression on the twin's powers")
                if grid.size:
                    bar = PW.BAR * scale * float(grid.max()) * float(np.abs(bank[2]).max())
                    err = float(np.abs(g[c][..., 0].astype(np.float64) - numpy_of(want)[..., 0]).max())
                    assert err <= bar, (what, c, err, bar)
        else:
            rows = every_rows(n1, every, first)
            assert g[c].shape == (rows, band[1]) and g[c].dtype == np.dtype(fd), (what, c, g[c].shape)
            # (of a call staged in segments "last_chunks" is the last segment's: segments are calls in sequence, each of its own chunks)
            one_chunk = all(r["chunks"] == 1 and r["segments"] == 1 for r in cx.routes)
            end = None if cx.s0 is None else np.atleast_2d(cx.state_now)[c][None]
            if exact and (one_chunk or case["decay"] == 0):
                if case["decay"] == 0 and rows:              # promise (4): the power call's bits, on any chunking
                    SM.same_bits(g[c], np.ascontiguousarray(PW.on_grid(pw, every, first, band)), (what, c, "decay 0"))
                    RAN["power_smooth decay 0, bits" + ("" if one_chunk else ", several chunks")] += c == 0
                pieces = smooth_reference(cx, cols, c, SM.loop)
                if rows:
                    SM.same_bits(g[c], np.concatenate([r for r, _ in pieces])[first::every], (what, c))
                RAN["power_smooth the loop, bits"] += c == 0
                if end is not None:
                    SM.same_bits(end, pieces[-1][1][None], (what, c, "state"))
                    RAN["power_smooth the loop, state bits"] += c == 0
            else:
                pieces = smooth_reference(cx, cols, c, SM.wide)
                ref, big = (np.concatenate([r[i] for r in pieces]) for i in (0, 1))
                extra = 0.0 if exact else PW.BAR * scale * pmax
                if rows:
                    SM.within_bound(g[c], ref[first::every], big[first::every], pieces[0][2], (what, c), extra=extra)
                RAN["power_smooth the bound" + (" + BAR pmax" if extra else "")] += c == 0
                if end is not None:
                    SM.within_bound(end, ref[-1:], big[-1:], pieces[0][2], (what, c, "state"), extra=extra)
                    RAN["power_smooth the bound, state"] += c == 0


# ---------------------------------------------------------------------------------------------
# a case, either slate
# ---------------------------------------------------------------------------------------------
def run_case(case):
    kind, stratum, combo, m, ch = case["kind"], case["stratum"], case["combo"], case["m"], case["channels"]
    n0, n1, every, first, opts = case["n0"], case["n1"], case["every"], case["first"], case["opts"]
    second = kind in GC.KINDS2
    band = tuple(case["band"]) if "band" in case else None
    td, fd, fdx = O.combo_types(combo)
    loose = bool(opts.get("float_carry_parallel"))
    scale = LOOSE if loose else 1.0
    what = repr(case)
    if kind == "power_smooth":
        SM.need_wide(combo)
        assert case["decay"] in SM.DECAYS or case["decay"] == smooth_decay(case["tau"]), what
    n = n0 + n1 + GC.CLOSING
    x = XS.signals(td, n, case["xseed"], ch) if ch > 1 else PW.signal(n, td, case["xseed"])[None]
    x0, x1, x2 = (np.ascontiguousarray(v if ch > 1 else v[0]) for v in (x[:, :n0], x[:, n0:n0 + n1], x[:, n0 + n1:]))
    mode_exact = GC.exact_mode(case)
    parts = GC.parts(case)
    cx = types.SimpleNamespace(case=case, kind=kind, ch=ch, band=band, what=what, loose=loose, scale=scale, fd=fd, fdx=fdx, parts=parts,
                               mode_exact=mode_exact, staged="stage_bytes" in opts, x0=x0, x0in=PW.to_dev(x0) if case["device"] else x0,
                               installed=None, prev=None, s0=None, state_now=None)

    with new_plan(case) as p, new_plan(case, lists=False) as q:
        # the geometry the generator restates is the plan's
        lanes, bpl, per = GC.geometry(combo, case["window"], opts.get("interior", 0))
        assert (p.get_option("interior"), p.get_option("bins_per_lane"), p.get_option("tiles")) == (lanes, bpl, case["tiles"]), what
        assert per == case["per"] and bool(p.get_option("carry")) == mode_exact and p.get_option("test_hooks") == int(case["hooks"]), what

        # warm-up
        exact = True
        if stratum == "installed":
            with new_plan(case) as w:
                if n0:
                    call(w, case["warm"], x0, 7, 3, tuple(case["warm_band"]), case=case)
                acc, fid, hist, cursor = w.state()
            if case["fid_scale"]:
                factor = 2.0 ** np.arange(ch) if second else 1 + np.arange(ch) / 1024
                fid = fid * factor.astype(fid.real.dtype)[:, None]
                assert fid.dtype == fdx and not np.array_equal(fid[0], fid[1])
            p.set_state(acc, fid, hist, cursor)
            q.set_state(acc, fid, hist, cursor)
            cx.installed = (acc, fid, hist, cursor)
            assert mode_exact, what
        elif n0:
            call(p, case["warm"], cx.x0in, 7, 3, tuple(case["warm_band"]), case=case)
            exact = mode_exact or p.get_option("last_chunks") == 1
            q.sdft(x0)
            exact = exact and (mode_exact or q.get_option("last_chunks") == 1)
        assert p.get_option("cursor") == n0 % (2 * m), what

        # the oracle's rows of the call under test (the twin's, from the installed state, where a channel has a fid of its own)
        # and, for the lag products, the row before them: None for the zero row of a fresh plan
        refs = None
        last = [None] * ch
        twin_rows = q.sdft(PW.to_dev(x1))
        twin_exact = exact and (mode_exact or q.get_option("last_chunks") == 1)      # (the twin's state is the reference's bits, too)
        if case["fid_scale"]:
            X = twin_rows.cpu().numpy()                      # (channels > 1)
            if kind == "lag_sum" and n0:                     # the oracle's last warm-up row, scaled where the fid enters
                for c in range(ch):
                    row = O.best(m, case["window"], 1.0, combo).sdft(x[c, :n0])[-1].astype(fdx)
                    last[c] = row * fdx(2.0 ** c) if n0 % (2 * m) else row
        else:
            refs = [O.best(m, case["window"], 1.0, combo[:3] + "f64" if loose else combo) for _ in range(ch)]
            X = np.empty((ch, n1, m), dtype=fdx)
            for c, r in enumerate(refs):
                if n0:
                    last[c] = r.sdft(x[c, :n0])[-1].astype(fdx)
                X[c] = r.sdft(x[c, n0:n0 + n1])              # (float_carry_parallel: the FD double oracle's rows, rounded once)
        del twin_rows
        cx.X, cx.prev = X, last

        # the smoothed call's state: inside a larger array, on the host or the device
        state = None
        if kind == "power_smooth" and case["state"] != "none":
            shape = (ch, band[1]) if ch > 1 else (band[1],)
            cx.s0 = SM.some_state(fd, shape, case["sseed"])
            around = np.full(cx.s0.size + 2 * STATE_PAD, STATE_MARK, dtype=fd)
            around[STATE_PAD:STATE_PAD + cx.s0.size] = cx.s0.ravel()
            if case["state"] == "device":
                around = PW.to_dev(around)
            state = around[STATE_PAD:STATE_PAD + cx.s0.size].reshape(shape)

        # the call under test: one call, or two on one grid
        outs, cx.routes, cx.xins = [], [], []
        arena = out = None
        t = 0
        for part in parts:
            shape, dtype = output_shape(part, p)
            xs = np.ascontiguousarray(x1[..., t:t + part["n1"]])
            t += part["n1"]
            xin = PW.to_dev(xs) if case["device"] else xs
            if case["out"] is not None and math.prod(shape) > 0:
                arena = G.DeviceArena(G.room((shape, dtype)))
                out = arena.carve(shape, dtype, case["out"][0], case["out"][1], name=kind)
                assert G.ptr_of(out) % case["out"][1] == case["out"][0] % case["out"][1]
            got = call(p, kind, xin, every, part["first"], band, out=out, case=case, state=state)
            cx.routes.append(route_of(p))
            cx.xins.append(xin)
            if arena is not None:
                arena.check()
                assert G.view_unwritten(out) == 0, what
            got = numpy_of(got)
            assert got.shape == shape and got.dtype == np.dtype(dtype), (what, got.shape, shape)
            outs.append(got)
        assert (arena is None or len(parts) == 1) and t == n1, what
        route = cx.routes[0]
        exact = exact and all(mode_exact or r["chunks"] == 1 for r in cx.routes) and not loose
        cx.exact = exact
        TALLY[(kind, stratum, route["chain"], "1" if route["chunks"] == 1 else "2" if route["chunks"] == 2 else "3+")] += 1
        if state is not None:
            around = numpy_of(around)
            cx.state_now = around[STATE_PAD:STATE_PAD + cx.s0.size].reshape(cx.s0.shape)
            assert (around[:STATE_PAD] == STATE_MARK).all() and (around[STATE_PAD + cx.s0.size:] == STATE_MARK).all(), (what, "around the state")

        # the route (of a split case: the first call's; the second's kernel and forced chunk length)
        one = parts[0]
        assert all(r["kernel"] == GC.KERNEL[kind] for r in cx.routes), (what, cx.routes)
        if stratum == "one_chunk":
            assert all(r["chunks"] == 1 for r in cx.routes), (what, cx.routes)
        if stratum == "relay":
            assert route["chain"] == 3 and route["chunks"] > 1 and exact, (what, route)
        if stratum in ("serial", "sums", "installed"):
            assert route["chain"] == 0 and route["chunks"] > 1 and exact == (stratum != "sums"), (what, route)
        if stratum == "segments":
            assert route["segments"] == 3 and exact, (what, route)
        if opts.get("chunk", 0) > 0 and not cx.staged:
            assert all(r["chunk_len"] == GC.chunk_len_of(part) for part, r in zip(parts, cx.routes)), (what, cx.routes)
            cuts = GC.chunk_cuts(one)
            assert route["chunks"] == len(cuts) or stratum == "free", (what, route, len(cuts))

        # the values
        if second:
            join = {"power_peak": PK.join_of(case.get("hold", "max")), "lag_sum": np.add, "power_moments": np.add}.get(kind)
            cx.g = joined(cx, outs, kind in GC.POOLED, join)
            check_second(cx)
        else:
            cx.g = joined(cx, outs, False)
            check_first(cx)

        # the state, all channels, and the closing hop
        check_state(p, q, exact and twin_exact, LOOSE_ROW_BAR if loose else 1e-10, what)
        g2 = p.sdft(x2)
        exact = exact and (mode_exact or p.get_option("last_chunks") == 1)      # (a forced chunk shorter than the hop cuts it, too)
        if refs is None:
            w2 = q.sdft(x2)
        else:
            w2 = np.stack([r.sdft(x[c, n0 + n1:]) for c, r in enumerate(refs)]).astype(fdx)
            w2 = w2 if ch > 1 else w2[0]
        if exact:
            assert np.array_equal(g2, w2), (what, "closing hop")
        else:
            assert PW.rel(g2, w2) <= (LOOSE_ROW_BAR if loose else 1e-11), (what, "closing hop", PW.rel(g2, w2))


def tally_line(seed):
    """(kind, stratum, last_chain, chunks) of every call under test so far: the last seed's line is the run's tally (pytest -s)"""
    print("TALLY", seed, dict(sorted((" ".join(map(str, k)), v) for k, v in TALLY.items())))
    if RAN:
        print("CHECKS", seed, dict(sorted(RAN.items())))


@pytest.mark.parametrize("seed", range(40))
def test_random_grid_call_parity(seed):
    drawn = GC.cases(seed)
    ran = 0
    for case in drawn:
        run_case(case)
        ran += 1
    assert ran == len(drawn) == 7                            # the sweep skips no case
    tally_line(seed)


@pytest.mark.parametrize("seed", range(40))
def test_random_grid_call_parity_2(seed):
    drawn = GC.cases2(seed)
    ran = 0
    for case in drawn:
        run_case(case)
        ran += 1
    assert ran == len(drawn) == 7                            # the sweep skips no case
    tally_line(seed)
