"""Seeded, stratified sweep of the six grid analysis calls (sdft_hip_sdft_every_n, _power_n, _power_sum_n, _filterbank_n,
_cross_sum_n, _covariance_n) over the sizes, grids, bands and routes nobody picked by hand, on a real MI355X.  tests/grid_cases.py
draws the cases (seven per seed; its docstring describes the strata); a campaign beyond the committed seeds is
SDFT_FUZZ_OFFSET=1000 pytest tests/test_gpu_fuzz_grid.py -s, and a failure's message is the whole case.

A case is a warm-up call of n0 samples through a drawn entry point (it moves the cursor, and with it chunk_shift), the call under
test on the next n1 samples, and a closing sdft of 60 samples.  Each channel's stream goes through the oracle, call by call;
what numpy derives from the oracle's rows of the call is the expectation, by the helpers and bars of the call's own suite:

    every        the rows on the grid                           test_gpu_every.check         bits, or 1e-11 of the largest bin
    power        power_of(rows) on the grid and the band        test_gpu_power.check         bits, or BAR
    power_sum    wide-precision window sums of those powers     test_gpu_power_sum.check     gamma_L, + L BAR pmax when inexact
    filterbank   reference(bank, powers)                        test_gpu_filterbank.check_rows
    cross_sum,   numpy's unfused terms, summed per window       test_gpu_cross_sum.check_pairs (at (1, 0) on exact routes: the
    covariance                                                                                terms' bits)

A case is exact where test_gpu_fuzz.py says a call is -- FD float without float_carry_parallel, carry = 1, or a call of one time
chunk -- for the warm-up AND the call under test: an inexact warm-up leaves a state off by rounding.  On exact pair cases every
(b, a) is the conjugate of its (a, b), auto-pairs have im == +0, and the covariance call has the bits of the cross-spectrum call
of a twin plan that is given the same chunk length (as test_covariance_wide_array does).

FD float with float_carry_parallel = 1 (the stratum `sums`) is the one route none of the grid suites states a bar for: its rows
differ from the float oracle's by float rounding, so the 1e-11 of FD double's fast carries cannot apply.  What the project
promises of that option is tests/test_gpu_parity.py test_float_plans_with_chunk_parallel_carries: within 1e-4 of the
double-precision reference, relative to the largest bin.  So there the oracle is the FD double one of the same TD (its rows rounded
to float once), the row bar is 1e-4 in place of 1e-11, and the inexact terms of the helpers -- all of them BAR = 2.1 x the row bar
times a scale -- are scaled by 1e-4 / 1e-11 through the scale arguments the helpers already take; the state and the closing hop
are held to 1e-4 likewise.  Nothing else about the checks changes.

With a fid of its own per channel (stratum `installed`, batched plans of every second pair of seeds) the oracle cannot follow:
the rows are those a twin plan's sdft gives from the same installed state, as
test_cross_sum_after_a_state_with_a_fid_of_its_own_per_channel has it.

After every case: the state of all channels against a twin that ran sdft alone (bits on exact routes, 1e-10 otherwise), the
closing hop against the oracle (bits, 1e-11), the kernel, the stratum's carry form, and a forced chunk length honoured.  One case
in three hands the call an output carved from a guarded arena at a drawn residue: no byte outside it is written, none inside left."""

import collections
import math

import numpy as np
import pytest

import grid_cases as GC
import guarded as G
import test_gpu_cross_sum as XS
import test_gpu_cross_sum_routes as XR
import test_gpu_every as EV
import test_gpu_filterbank as FB
import test_gpu_power as PW
import test_gpu_power_sum as PS
from oracle import oracle as O
from sdft_amd.sdft import SDFT, covariance_pairs, every_rows, power_sum_rows

pytestmark = pytest.mark.gpu
LOOSE_ROW_BAR, ROW_BAR = 1e-4, EV.BAR                        # float_carry_parallel (tests/test_gpu_parity.py); FD double's fast carries
LOOSE = LOOSE_ROW_BAR / ROW_BAR                              # what the helpers' inexact scales are multiplied by on that route
assert ROW_BAR == 1e-11 and PW.BAR == 2.1 * ROW_BAR
assert GC.COMBOS == O.COMBOS and GC.PAIRS == XS.PAIRS and GC.PAIR_LISTS == FB.PAIR_LISTS and GC.ARRAY_LISTS == FB.ARRAY_LISTS
assert GC.WRITER_LISTS == XR.WRITER_LISTS and tuple(GC.WINDOWS) == tuple(PW.WINDOWS)
TALLY = collections.Counter()                                # (kind, stratum, last_chain, chunks) of the calls under test of this run


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
    """random_bands(m) as the filterbank suite draws them, plus the case's bands that end or begin on a tile boundary"""
    start, length, w = FB.random_bands(case["m"], 1000 + case["bank"]["seed"])
    extra = case["bank"]["extra"]
    if extra:
        rng = np.random.default_rng(case["bank"]["seed"])
        start = np.concatenate([start, np.array([b for b, _ in extra], dtype=np.uint64)])
        length = np.concatenate([length, np.array([k for _, k in extra], dtype=np.uint64)])
        w = np.concatenate([w, rng.uniform(2.0 ** -10, 1.0, sum(k for _, k in extra))])
    return FB.in_fd((start, length, w), fd)


def install(p, case):
    if case["kind"] == "filterbank":
        p.set_filterbank(*bank_of(case, p.fd))
    if case["kind"] == "cross_sum":
        p.set_pairs([a for a, _ in case["pairs"]], [b for _, b in case["pairs"]])
        assert p.pairs == len(case["pairs"])
    if case["kind"] == "covariance":
        p.set_array(case["array"])
        assert p.array_channels == len(case["array"])


def call(p, name, x, every, first, band, out=None):
    if name == "sdft":
        return p.sdft(x)
    if name == "every":
        return p.sdft_every(x, every, first, out=out)
    if name == "filterbank":
        return p.filterbank(x, every, first, out=out)
    return getattr(p, name)(x, every, first, bins=band, out=out)


def output_shape(case, p):
    n1, every, first, ch = case["n1"], case["every"], case["first"], case["channels"]
    kind = case["kind"]
    lead = (ch,) if ch > 1 else ()
    if kind == "every":
        return lead + (every_rows(n1, every, first), case["m"]), p.fdx
    if kind == "power":
        return lead + (every_rows(n1, every, first), case["band"][1]), p.fd
    if kind == "power_sum":
        return lead + (power_sum_rows(n1, every, first), case["band"][1]), p.fd
    if kind == "filterbank":
        return lead + (every_rows(n1, every, first), p.filterbank_bands), p.fd
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
    """all channels, whether or not a pair or an array names them"""
    a, b = p.state(), q.state()
    assert a[3] == b[3] and np.array_equal(a[2], b[2]), what
    for name, u, v in (("acc", a[0], b[0]), ("fid", a[1], b[1])):
        u, v = np.atleast_2d(u), np.atleast_2d(v)
        for c in range(u.shape[0]):
            if exact:
                assert XS.same_bits(u[c].copy(), v[c].copy()), (what, name, c)
            else:
                assert PW.rel(u[c], v[c]) <= bar, (what, name, c, PW.rel(u[c], v[c]))


def run_case(case):
    import torch
    kind, stratum, combo, m, ch = case["kind"], case["stratum"], case["combo"], case["m"], case["channels"]
    n0, n1, every, first, opts = case["n0"], case["n1"], case["every"], case["first"], case["opts"]
    band = tuple(case["band"]) if "band" in case else None
    td, fd, fdx = O.combo_types(combo)
    loose = bool(opts.get("float_carry_parallel"))
    scale = LOOSE if loose else 1.0
    what = repr(case)
    n = n0 + n1 + GC.CLOSING
    x = XS.signals(td, n, case["xseed"], ch) if ch > 1 else PW.signal(n, td, case["xseed"])[None]
    x0, x1, x2 = (np.ascontiguousarray(v if ch > 1 else v[0]) for v in (x[:, :n0], x[:, n0:n0 + n1], x[:, n0 + n1:]))
    mode_exact = GC.exact_mode(case)

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
                    call(w, case["warm"], x0, 7, 3, tuple(case["warm_band"]))
                acc, fid, hist, cursor = w.state()
            if case["fid_scale"]:
                fid = fid * (1 + np.arange(ch) / 1024).astype(fid.real.dtype)[:, None]
                assert fid.dtype == fdx and not np.array_equal(fid[0], fid[1])
            p.set_state(acc, fid, hist, cursor)
            q.set_state(acc, fid, hist, cursor)
            assert mode_exact, what
        elif n0:
            call(p, case["warm"], PW.to_dev(x0) if case["device"] else x0, 7, 3, tuple(case["warm_band"]))
            exact = mode_exact or p.get_option("last_chunks") == 1
            q.sdft(x0)
            exact = exact and (mode_exact or q.get_option("last_chunks") == 1)
        assert p.get_option("cursor") == n0 % (2 * m), what

        # the oracle's rows of the call under test (the twin's, from the installed state, where a channel has a fid of its own)
        refs = None
        twin_rows = q.sdft(PW.to_dev(x1))
        twin_exact = exact and (mode_exact or q.get_option("last_chunks") == 1)      # (the twin's state is the reference's bits, too)
        if case["fid_scale"]:
            X = twin_rows.cpu().numpy()                      # (channels > 1)
        else:
            refs = [O.best(m, case["window"], 1.0, combo[:3] + "f64" if loose else combo) for _ in range(ch)]
            X = np.empty((ch, n1, m), dtype=fdx)
            for c, r in enumerate(refs):
                if n0:
                    r.sdft(x[c, :n0])
                X[c] = r.sdft(x[c, n0:n0 + n1])              # (float_carry_parallel: the FD double oracle's rows, rounded once)
        del twin_rows

        # the call under test
        shape, dtype = output_shape(case, p)
        xin = PW.to_dev(x1) if case["device"] else x1
        arena = out = None
        if case["out"] is not None and math.prod(shape) > 0:
            arena = G.DeviceArena(G.room((shape, dtype)))
            out = arena.carve(shape, dtype, case["out"][0], case["out"][1], name=kind)
            assert G.ptr_of(out) % case["out"][1] == case["out"][0] % case["out"][1]
        got = call(p, kind, xin, every, first, band, out=out)
        route = {k: p.get_option("last_" + k) for k in ("kernel", "chunks", "chunk_len", "chain", "segments")}
        exact = exact and (mode_exact or route["chunks"] == 1) and not loose
        if arena is not None:
            arena.check()
            assert G.view_unwritten(out) == 0, what
        got = numpy_of(got)
        assert got.shape == shape and got.dtype == np.dtype(dtype), (what, got.shape, shape)
        TALLY[(kind, stratum, route["chain"], "1" if route["chunks"] == 1 else "2" if route["chunks"] == 2 else "3+")] += 1

        # the route
        staged = "stage_bytes" in opts
        assert route["kernel"] == GC.KERNEL[kind], (what, route)
        if stratum == "one_chunk":
            assert route["chunks"] == 1, (what, route)
        if stratum == "relay":
            assert route["chain"] == 3 and route["chunks"] > 1 and exact, (what, route)
        if stratum in ("serial", "sums", "installed"):
            assert route["chain"] == 0 and route["chunks"] > 1 and exact == (stratum != "sums"), (what, route)
        if stratum == "segments":
            assert route["segments"] == 3 and exact, (what, route)
        if opts.get("chunk", 0) > 0 and not staged:
            assert route["chunk_len"] == GC.chunk_len_of(case), (what, route)
            cuts = GC.chunk_cuts(case)
            assert route["chunks"] == len(cuts) or stratum == "free", (what, route, len(cuts))

        # the values
        g = got if (ch > 1 or kind in ("cross_sum", "covariance")) else got[None]
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
            if kind == "covariance" and mode_exact and not staged:
                # the cross-spectrum call of a twin plan from the same state, given the covariance call's chunk length: the same bits
                with new_plan(case, lists=False) as t:
                    if stratum == "installed":
                        t.set_state(acc, fid, hist, cursor)
                    elif n0:
                        t.sdft(x0)
                    t.set_pairs([a for a, _ in pairs], [b for _, b in pairs])
                    t.set_option("chunk", route["chunk_len"])
                    same = numpy_of(t.cross_sum(xin, every, first, bins=band))
                    assert (t.get_option("last_kernel"), t.get_option("last_chunk_len"), t.get_option("last_chunks")) == (8, route["chunk_len"], route["chunks"]), what
                    assert XS.same_bits(g, same), (what, "covariance against cross_sum")

        # the state, all channels, and the closing hop
        check_state(p, q, exact and twin_exact, LOOSE_ROW_BAR if loose else 1e-10, what)
        g2 = p.sdft(x2)
        if refs is None:
            w2 = q.sdft(x2)
        else:
            w2 = np.stack([r.sdft(x[c, n0 + n1:]) for c, r in enumerate(refs)]).astype(fdx)
            w2 = w2 if ch > 1 else w2[0]
        if exact:
            assert np.array_equal(g2, w2), (what, "closing hop")
        else:
            assert PW.rel(g2, w2) <= (LOOSE_ROW_BAR if loose else 1e-11), (what, "closing hop", PW.rel(g2, w2))


@pytest.mark.parametrize("seed", range(40))
def test_random_grid_call_parity(seed):
    drawn = GC.cases(seed)
    ran = 0
    for case in drawn:
        run_case(case)
        ran += 1
    assert ran == len(drawn) == 7                            # the sweep skips no case
    # (kind, stratum, last_chain, chunks) of every call under test so far: the last seed's line is the run's tally (pytest -s)
    print("TALLY", seed, dict(sorted((" ".join(map(str, k)), v) for k, v in TALLY.items())))
