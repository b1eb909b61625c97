"""Every entry point on guarded, misaligned caller buffers (tests/guarded.py).

Every case runs ONE call pattern on fresh plans with the same options: once on ordinary buffers (torch.empty / .cuda() /
fresh numpy arrays: 256-byte aligned or better), then once per PLACEMENT with every caller buffer carved from a guarded
arena, one buffer at a time at every residue modulo 16 its element size allows (TD float 4, 8, 12; TD double 8; complex64 8;
complex128 none), once 16-byte but not 128-byte aligned (data_ptr() % 128 in {16, 80}), and once with everything off.
Each run asserts
  1. arena.check() and view_unwritten == 0: no store outside [ptr, ptr + count), no hole; the inputs keep their bits;
  2. the oracle (oracle.best): bit-identical where the project claims it (FD float, carry = 1, calls of one chunk, synthesis
     with exact_inverse = 1, the fused call with the reference's order), else the criterion of test_gpu_exact.py (exact_sdft:
     check_bins / check_pipeline / check_samples with their floors) on sampled rows including the first and last of a call;
  3. outputs and state() (accumulators, fiddles, delay line, cursor) of the guarded run equal the aligned run's bit for bit:
     alignment selects loads and stores, never arithmetic.  No route was found where that is legitimately false: the forks on
     the address (vec_store, the bin-pair kernel, ordered rows) all lead to kernels that are bit-identical by design;
  4. the route intended was the route taken (get_option last_*), on the aligned and on the guarded run.

The 16-byte global accesses on CALLER memory and what keeps each off a misaligned address (sdft_amd/csrc):
  sdft_forward.hpp:535         tile kernel, FD float pair store (V = 4 floats): ForwardArgs::vec_store, which
                               logic::forward_route (sdft_plan_logic.hpp:677) clears unless out % 16 == 0, nbins and the
                               channel stride are even and there is no row-pointer table; otherwise two 8-byte stores.
                               :550 (FD double) stores ONE complex128 = 16 bytes: element-aligned means 16-byte aligned.
  sdft_forward_rows.hpp:314, :329      row-group kernel: the same two cases under the same vec_store.
  sdft_forward_hop.hpp:146, :161, :496, :511   hop kernel and the hop of the fused call: vec_store as computed by
                               sdft_plan.hpp:1106 (same predicate, repeated) -- :161 / :511 are the FD double element store.
  sdft_forward_every.hpp:120, :135     decimated analysis: vec_store from forward_route (q.out is the kept-rows matrix).
  sdft_resident.hpp:144        the resident kernel recomputes vec_store from the row pointer of each call.
  sdft_forward_rows_f32.hpp:249        bin-pair kernel: 16-byte stores always; taken only when rows_f32 holds, which
                               requires vec_store (sdft_plan_logic.hpp:679), so never on a misaligned matrix.
                               :117-119 and :312-313 load the plan's own tables (tw, carry), not caller memory.
  sdft_inverse.hpp:477         ordered-rows synthesis, 16-byte loads only: logic::rows_ordered_ok (sdft_plan_logic.hpp:741)
                               declines unless (in & 15) == 0 (and nbins is even at FD float).
  sdft_inverse.hpp:715         row kernel (one wave per row): vec_ok at :693 tests ((uintptr_t)row & 15) == 0 per row.
  sdft_inverse.hpp:54          load_bin: one complex bin (8 or 16 bytes), element-aligned.
  sdft_inverse.hpp:604         streaming synthesis: vec_ok (:574) looks at nbins, the row-pointer table and the channel
                               stride, NOT at the base.  At FD float a matrix 8 bytes past a 16-byte boundary is therefore
                               read with 16-byte FLAT loads at addresses that are only 8-byte aligned: a plain global access
                               on caller memory.  gfx950 serves it (unaligned access mode; test_gpu_parity.py's misaligned
                               leg and the cases below show the right bits); whether it costs bandwidth has not been
                               measured, so nothing is claimed about it.
  sdft_copy_engine.hpp:48      host-side copy: scalar head until dst is 16-byte aligned, 16-byte body, scalar tail.
Everything else that touches caller memory (samples, gain vectors, dfts of the fused call outside the cases above) is an
element-sized access.  vec_store itself has no observer: where rows are a multiple of 128 bins last_rows_f32 shows it
(1 aligned, 0 eight bytes off); elsewhere the scalar-store branch follows from the address by the predicate above, which
tests/cpp/plan_logic_test.cpp checks on the CPU.
"""

import ctypes as C

import numpy as np
import pytest

import exact_sdft as X
import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import every_next_first, every_rows

import test_gpu_exact as TE            # signal(), call_rows(), op_kwargs(), lipschitz(), model_op(): shared helpers

pytestmark = pytest.mark.gpu


# ---- placements ---------------------------------------------------------------------------------------------------------------
def residues(dtype):
    """The non-zero residues modulo 16 an element of this type can sit at."""
    size = np.dtype(dtype).itemsize
    return tuple(range(size, 16, size)) if size < 16 else ()


def placements(bufs, wide=None):
    """bufs: {name: dtype} of a call's buffers -> list of {name: residue | (residue, modulus)}: all on 16 bytes, one buffer
    at a time at each non-zero residue, `wide` 16 bytes past a 128-byte boundary, everything off (a type without a
    non-zero residue: 80 bytes past a 128-byte boundary)."""
    out = [{}]
    for name, dt in bufs.items():
        out += [{name: r} for r in residues(dt)]
    if wide:
        out.append({wide: (16, 128)})
    out.append({name: (max(residues(dt)) if residues(dt) else (80, 128)) for name, dt in bufs.items()})
    return out


def off16(where, name) -> bool:
    """Is buffer `name` off a 16-byte boundary in this placement?"""
    r = (where or {}).get(name, 0)
    return (r[0] if isinstance(r, tuple) else r) % 16 != 0


def tag(where):
    return "aligned" if where is None else "guarded " + (",".join(f"{k}@{v}" for k, v in where.items()) or "@0")


# ---- buffers of a call ----------------------------------------------------------------------------------------------------------
class Call:
    def __init__(self, arena, views, specs):
        self.arena, self.v, self.specs = arena, views, specs

    def __getitem__(self, name):
        return self.v[name]

    def check(self, outputs, what=""):
        """Assertion 1: guards intact, outputs completely written, inputs untouched."""
        if self.arena is None:
            return
        self.arena.check()
        for name, shape, dtype, values in self.specs:
            if name in outputs:
                holes = G.view_unwritten(self.v[name])
                assert holes == 0, (what, name, "elements never written", holes)
            elif values is not None:
                assert same_bits(G.to_numpy(self.v[name]), np.asarray(values, dtype=dtype).reshape(shape)), (what, name, "input changed")


class Buffers:
    """The buffers of a run's calls: plain (where is None) or carved from one guarded arena per call; kept alive for the run."""

    def __init__(self, where, host=False):
        self.where, self.host, self.keep = where, host, []

    def call(self, specs):
        """specs: (name, shape, dtype, values or None for an output)"""
        import torch
        views = {}
        if self.where is None:
            for name, shape, dtype, values in specs:
                if self.host:
                    views[name] = np.array(values, dtype=dtype).reshape(shape) if values is not None else np.empty(shape, dtype=dtype)
                elif values is not None:
                    views[name] = torch.from_numpy(np.ascontiguousarray(values, dtype=dtype).reshape(shape)).cuda()
                else:
                    views[name] = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
            c = Call(None, views, specs)
        else:
            arena = (G.HostArena if self.host else G.DeviceArena)(G.room(*[(shape, dtype) for _, shape, dtype, _ in specs]))
            for name, shape, dtype, values in specs:
                r = self.where.get(name, 0)
                r, mod = r if isinstance(r, tuple) else (r, 16)
                views[name] = arena.carve(shape, dtype, r, mod, name=name)
                if values is not None:
                    G.put(views[name], values)
            c = Call(arena, views, specs)
        self.keep.append(c)
        return c


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def make(N, window="hann", latency=1.0, combo="f32f64", channels=1, **opts):
    from sdft_amd.sdft import SDFT
    p = SDFT(N, window, latency, combo, channels)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def same_run(base, got, what):
    """Assertion 3: outputs and state of a guarded run against the aligned run, bit for bit."""
    assert len(base["outs"]) == len(got["outs"])
    for i, (a, b) in enumerate(zip(base["outs"], got["outs"])):
        assert same_bits(a, b), (what, "call", i, "differs from the aligned run", int((np.asarray(a) != np.asarray(b)).sum()))
    for name, a, b in zip(("acc", "fid", "hist"), base["state"][:3], got["state"][:3]):
        assert same_bits(a, b), (what, "state", name)
    assert base["state"][3] == got["state"][3], (what, "cursor")


def state_is_the_oracles(state, refs, what):
    acc, fid, hist, cur = state
    for c, r in enumerate(refs):
        racc, rfid, rhist, rcur = r.state()
        pick = (lambda a: a[c]) if len(refs) > 1 else (lambda a: a)
        assert cur == rcur and np.array_equal(pick(acc), racc) and np.array_equal(pick(fid), rfid) and np.array_equal(pick(hist), rhist), (what, "state", c)


# ---- analysis: sdft_sdft_n / sdft_hip_sdft_every_n -----------------------------------------------------------------------------
def analysis_case(combo, N, lengths, opts, expect, exact, window="hann", channels=1, every=None, first=0, host=False, seed=1, places=None):
    """Calls of `lengths` samples, aligned and at every placement.  expect(p, i, where) asserts the route of call i.
    every: decimated analysis on one row grid over the calls (first: of the first call)."""
    td, fd, fdx = O.combo_types(combo)
    n = int(sum(lengths))
    xs = np.stack([TE.signal(n, seed + 17 * c, td) for c in range(channels)])
    refs = [O.best(N, window, 1.0, combo) for _ in range(channels)]
    full = [r.sdft(xs[c]) for c, r in enumerate(refs)]                         # the oracle's rows of the whole stream
    firsts, kept, t0, f = [], [], 0, first
    for n1 in lengths:
        firsts.append(f)
        kept.append(np.arange(t0 + f, t0 + n1, every) if every else np.arange(t0, t0 + n1))
        if every:
            f = every_next_first(n1, every, f)
        t0 += n1

    def run(where):
        what = (combo, N, window, opts, tag(where))
        with make(N, window, 1.0, combo, channels, **opts) as p:
            bufs, outs, geo, t0 = Buffers(where, host), [], [], 0
            for i, n1 in enumerate(lengths):
                part = xs[:, t0:t0 + n1] if channels > 1 else xs[0, t0:t0 + n1]
                rows = len(kept[i])
                shape = (rows, N) if channels == 1 else (channels, rows, N)
                c = bufs.call([("x", part.shape, td, part), ("out", shape, fdx, None)])
                if every:
                    assert every_rows(n1, every, firsts[i]) == rows
                    p.sdft_every(c["x"], every, firsts[i], out=c["out"] if rows else None)      # rows == 0: dfts = NULL
                else:
                    p.sdft(c["x"], out=c["out"])
                expect(p, i, where)
                c.check({"out"}, what + (i,))
                outs.append(G.to_numpy(c["out"]))
                geo.append((p.get_option("last_chunks"), p.get_option("last_chunk_len")))
                t0 += n1
            return dict(outs=outs, state=p.state(), geo=geo)

    def verify(res, where):
        what = (combo, N, window, opts, tag(where))
        for c in range(channels):
            for i, o in enumerate(res["outs"]):
                oc = o[c] if channels > 1 else o
                if exact:
                    assert np.array_equal(oc, full[c][kept[i]]), (what, "call", i, "channel", c)
        if exact:
            state_is_the_oracles(res["state"], refs, what)
            return
        J, Lc = max(g[0] for g in res["geo"]), max(g[1] for g in res["geo"])
        rng = np.random.default_rng(seed)
        picks, t0 = [], 0                                                         # (call, index into the call's kept rows)
        for i, n1 in enumerate(lengths):
            if every:
                picks += [(i, j) for j in range(len(kept[i]))]
            else:
                picks += [(i, t - t0) for t in sorted(TE.call_rows(N, t0, n1, res["geo"][i][1], res["geo"][i][0], rng))]
            t0 += n1
        rows = np.array([kept[i][j] for i, j in picks])
        for c in range(channels):
            st = X.Stream(xs[c], N, combo)
            Zx = st.rows(rows, window)
            Zp = np.stack([(res["outs"][i][c] if channels > 1 else res["outs"][i])[j] for i, j in picks])
            F = X.analysis_floor(combo, N, st.A(rows), J, Lc)
            X.check_bins(X.bin_errors(Zp, Zx), X.bin_errors(full[c][rows], Zx), F, what=what + (c,))
            ax = st.acc(n - 1)
            a_gpu = res["state"][0][c] if channels > 1 else res["state"][0]
            e_gpu = float(np.abs(a_gpu.astype(X.CLD) - ax).max())
            e_ref = float(np.abs(refs[c].state()[0].astype(X.CLD) - ax).max())
            assert e_gpu <= X.C_FACTOR * max(e_ref, 2 * N * F), ("state", what, c, e_gpu, e_ref, 2 * N * F)

    base = run(None)
    verify(base, None)
    for where in (places if places is not None else placements({"x": td, "out": fdx}, wide="out")):
        got = run(where)
        verify(got, where)
        same_run(base, got, (combo, N, opts, tag(where)))


def opt(p, **want):
    for k, v in want.items():
        got = p.get_option(k)
        assert (got in v) if isinstance(v, (tuple, set)) else (got == v), (k, got, v)


def rows_f32(p, where, N, combo):
    """FD float rows of a multiple of 128 bins: the bin-pair kernel on an aligned matrix, the generic row-group kernel 8 bytes off."""
    if combo.endswith("f32") and N % 128 == 0 and p.get_option("last_kernel") == 2:
        opt(p, last_rows_f32=0 if off16(where, "out") else 1)
    elif p.get_option("last_kernel") == 2:
        opt(p, last_rows_f32=0)


EXACT_GEOMETRIES = [("f32f32", 1000), ("f64f32", 127), ("f32f64", 1025), ("f64f64", 128), ("f32f32", 4096), ("f32f64", 2048), ("f32f32", 1024),
                    ("f64f64", 7)]


@pytest.mark.parametrize("combo,N", EXACT_GEOMETRIES)
@pytest.mark.parametrize("rows_kernel", [0, 1])
def test_analysis_tiles_and_row_groups_exact_carries(combo, N, rows_kernel):
    """Independent tiles (last_kernel 1; hooks library, rows_kernel = 0) and row groups (2, two slots per lane at N = 2048 double /
    4096 float), exact carries: a ragged last chunk, then a call shorter than the chunk through the general launches (hop_kernel 0)."""
    def expect(p, i, where):
        kernel = 2 if rows_kernel and N >= 8 else 1
        opt(p, last_kernel=kernel, last_chunks=(4, 1)[i], carry=1)
        rows_f32(p, where, N, combo)
    analysis_case(combo, N, [1 * 504 * 3 + 77, 401], dict(chunk=504, carry=1, rows_kernel=rows_kernel, hop_kernel=0), expect, True,
                  window=("hann", "blackman", "hamming", "boxcar")[N % 4], seed=N)


@pytest.mark.parametrize("N", [1025, 2048, 127, 1000])
@pytest.mark.parametrize("rows_kernel", [0, 1])
def test_analysis_tiles_and_row_groups_chunk_parallel(N, rows_kernel):
    """The same two kernels with carries from the pre-pass at FD double (not bit-exact by design: per bin against the model)."""
    def expect(p, i, where):
        opt(p, last_kernel=2 if rows_kernel else 1, last_self=0, carry=0, last_chain=0)
        assert p.get_option("last_chunks") > 1
    analysis_case("f32f64", N, [2 * N + 1503, 777], dict(chunk=500, carry=0, self_carry=0, rows_kernel=rows_kernel), expect, False,
                  window="blackman", seed=N)


@pytest.mark.parametrize("combo,N", [("f32f32", 7), ("f32f32", 1000), ("f32f32", 4096), ("f64f32", 127), ("f64f32", 128), ("f32f64", 2048),
                                     ("f32f64", 1025), ("f64f64", 1024)])
def test_analysis_hop_kernel(combo, N):
    """Calls of one time chunk (n < 512): the fused hop launch (last_kernel 3), bit-identical, in a stream of uneven hops."""
    def expect(p, i, where):
        opt(p, last_kernel=3, last_chunks=1)
    analysis_case(combo, N, [300, 37, 411, 1], {}, expect, True, window="hamming", seed=N)


@pytest.mark.parametrize("combo,N", [("f32f32", 1024), ("f32f32", 4096), ("f64f32", 128), ("f32f32", 2048)])
def test_analysis_bin_pair_kernel_and_its_fallback(combo, N):
    """FD float, N % 128 == 0, default options: forward_rows_f32_kernel on an aligned matrix (last_rows_f32 1), the generic
    row-group kernel with the scalar-store branch on a matrix 8 bytes past a 16-byte boundary (0) -- same bits."""
    seen = set()

    def expect(p, i, where):
        opt(p, last_kernel=2, carry=1)
        assert p.get_option("last_chunks") > 1
        opt(p, last_rows_f32=0 if off16(where, "out") else 1)
        seen.add(p.get_option("last_rows_f32"))
    analysis_case(combo, N, [2200 + N // 8, 1111], {}, expect, True, window="blackman", seed=N)
    assert seen == {0, 1}


@pytest.mark.parametrize("combo,N,chunk", [("f32f64", 1024, 0), ("f64f64", 1000, 700), ("f32f64", 128, 0), ("f32f64", 2048, 512)])
def test_analysis_self_carried_chunks(combo, N, chunk):
    def expect(p, i, where):
        opt(p, last_self=1, last_kernel=2, carry=0)
        assert p.get_option("last_chunks") > 1
    analysis_case(combo, N, [2 * N + 3001, 2200], dict(chunk=chunk, carry=0), expect, False, seed=N)


@pytest.mark.parametrize("N,chunk,fft", [(1024, 512, 0), (1024, 512, 1), (1024, 512, 2), (1000, 704, 1), (127, 512, 0), (2048, 512, 1), (7, 304, 0)])
def test_analysis_prepass_carries(N, chunk, fft):
    """self_carry = 0: chunk partial sums by direct sums (fft_carry 0), the power-of-two FFT (1, 2), the mixed-radix FFT (N = 1000)."""
    def expect(p, i, where):
        opt(p, last_self=0, carry=0, last_chain=0)
        assert p.get_option("last_chunks") > 1
    analysis_case("f32f64", N, [2 * N + 3 * chunk + 5, 2 * chunk + 1], dict(chunk=chunk, carry=0, self_carry=0, fft_carry=fft), expect, False,
                  window=("hann", "blackman", "hamming", "boxcar")[(N + fft) % 4], seed=N + fft)


@pytest.mark.parametrize("combo,N,segments", [("f32f32", 128, 3), ("f32f64", 1024, 1), ("f64f32", 1025, 2), ("f64f64", 127, 1), ("f32f32", 4096, 1)])
def test_analysis_exact_serial_pass(combo, N, segments):
    """carry = 1, chain = 0: the serial carry pass (in time segments on the side stream), chunks of 200 samples, the last ragged."""
    def expect(p, i, where):
        opt(p, last_chain=0, carry=1, last_chunks=(9, 3)[i], last_segments=segments)
        rows_f32(p, where, N, combo)
    analysis_case(combo, N, [1677, 555], dict(chunk=200, carry=1, chain=0, segments=segments), expect, True, window="blackman", seed=N)


@pytest.mark.parametrize("combo,N,chunk", [("f32f32", 4096, 1024), ("f32f32", 1024, 0), ("f64f32", 512, 192), ("f32f64", 1024, 512), ("f64f64", 256, 96),
                                           ("f32f32", 2048, 128)])
@pytest.mark.parametrize("segments", [0, 3])
def test_analysis_exact_relay_form(combo, N, chunk, segments):
    """carry = 1, chain = 2 at the geometries of test_exact_carry_relay_form_long_blocks: a call from cursor 0, one that starts
    mid-block (the chunk grid shifts), flow mode (segments 0) and time segments."""
    def expect(p, i, where):
        opt(p, last_chain=3, carry=1, last_flow=0 if segments else 1)
        assert p.get_option("last_chunks") > 1
        rows_f32(p, where, N, combo)
    analysis_case(combo, N, [2 * max(chunk, 512) + 1061, 1500 + 63], dict(chunk=chunk, carry=1, chain=2, segments=segments), expect, True,
                  window="blackman", seed=N)


@pytest.mark.parametrize("combo,opts,exact", [("f32f64", dict(carry=0), False), ("f32f32", dict(chunk=512, chain=2), True),
                                              ("f64f64", dict(chunk=200, carry=1, rows_kernel=0), True)])
def test_analysis_batched_plan(combo, opts, exact):
    """Three channels in one plan: samples [3][n], matrix [3][n][N] -- every channel's rows, the stride between channels."""
    def expect(p, i, where):
        assert p.get_option("last_chunks") > 1
        if combo == "f32f64": opt(p, last_self=1)
        if combo == "f32f32": opt(p, last_chain=3)
        if combo == "f64f64": opt(p, last_kernel=1)
        rows_f32(p, where, 256, combo)
    analysis_case(combo, 256, [2100, 901], opts, expect, exact, channels=3, seed=5)


@pytest.mark.parametrize("combo,N,every,first,opts,exact", [
    ("f32f32", 1024, 100, 42, {}, True), ("f32f64", 1000, 997, 5, dict(carry=1), True), ("f64f32", 127, 1, 3, {}, True),
    ("f32f64", 1024, 100, 42, dict(carry=0), False), ("f64f64", 2048, 997, 600, dict(carry=1), True), ("f32f32", 4096, 100, 99, {}, True)])
def test_decimated_analysis(combo, N, every, first, opts, exact):
    """sdft_hip_sdft_every_n (last_kernel 4): only the kept rows are written, nothing past the last of them; a short call whose
    grid skips it keeps no row and is handed dfts = NULL (every = 997); the grid carries over from call to call."""
    lengths = [4100, 300, 700]

    def expect(p, i, where):
        if every == 1 and i > 0:
            opt(p, last_kernel=(2, 3))                                         # (every = 1 from first = 0 on is sdft_sdft_n itself)
        elif not (every == 997 and i == 1):                                    # (a call that keeps no row only advances the stream)
            opt(p, last_kernel=4)
    analysis_case(combo, N, lengths, opts, expect, exact, every=every, first=first, seed=every)
    if every == 997:
        f = every_next_first(lengths[0], every, first)
        assert every_rows(lengths[1], every, f) == 0                           # the case did hand a NULL matrix in


def test_decimated_analysis_batched():
    def expect(p, i, where):
        opt(p, last_kernel=4)
    analysis_case("f32f32", 128, [3000, 450], {}, expect, True, channels=3, every=100, first=7, seed=2)


def test_analysis_async_pipelined_into_two_matrices():
    """Asynchronous calls on the plan's own stream into two matrices carved from ONE arena (option pipeline): the checks run
    after synchronize()."""
    N, n, combo = 512, 13000, "f32f64"
    xs = TE.signal(2 * n, seed=9)
    ref = O.best(N, "hann", 1.0, combo)
    full = ref.sdft(xs)

    def run(where):
        import torch
        with make(N, "hann", 1.0, combo, **{"async": 1, "pipeline": 1}) as p:
            bufs = Buffers(where)
            c = bufs.call([("x0", (n,), np.float32, xs[:n]), ("x1", (n,), np.float32, xs[n:]), ("out0", (n, N), np.complex128, None),
                           ("out1", (n, N), np.complex128, None)])
            p.sdft(c["x0"], out=c["out0"])
            p.sdft(c["x1"], out=c["out1"])
            opt(p, last_pipelined=1, last_self=1)
            geo = (p.get_option("last_chunks"), p.get_option("last_chunk_len"))
            p.synchronize()
            torch.cuda.synchronize()
            c.check({"out0", "out1"}, tag(where))
            return dict(outs=[G.to_numpy(c["out0"]), G.to_numpy(c["out1"])], state=p.state(), geo=geo)

    def verify(res):
        rng = np.random.default_rng(4)
        J, Lc = res["geo"]
        rows = np.array(sorted(TE.call_rows(N, 0, n, Lc, J, rng) | TE.call_rows(N, n, n, Lc, J, rng)))
        st = X.Stream(xs, N, combo)
        Zx = st.rows(rows, "hann")
        Zp = np.stack([res["outs"][t // n][t % n] for t in rows])
        X.check_bins(X.bin_errors(Zp, Zx), X.bin_errors(full[rows], Zx), X.analysis_floor(combo, N, st.A(rows), J, Lc))

    base = run(None)
    verify(base)
    for where in ({}, {"x0": 4, "x1": 12, "out0": (16, 128), "out1": (80, 128)}):
        got = run(where)
        verify(got)
        same_run(base, got, tag(where))


# ---- synthesis: sdft_isdft_n ----------------------------------------------------------------------------------------------------
def synthesis_case(combo, N, n, latency, opts, expect, exact=True, channels=1, host=False, seed=3, places=None):
    """One synthesis call on the oracle's rows of a noisy sweep, aligned and at every placement of the matrix and the samples."""
    td, fd, fdx = O.combo_types(combo)
    xs = np.stack([TE.signal(n, seed + 5 * c, td) for c in range(channels)])
    d = np.stack([O.best(N, "hann", latency, combo).sdft(xs[c]) for c in range(channels)])
    want = np.stack([O.best(N, "hann", latency, combo).isdft(d[c]) for c in range(channels)])
    if channels == 1:
        d, want = d[0], want[0]

    def run(where):
        what = (combo, N, n, latency, opts, tag(where))
        with make(N, "hann", latency, combo, channels, **opts) as p:
            bufs = Buffers(where, host)
            c = bufs.call([("dfts", d.shape, fdx, d), ("y", want.shape, td, None)])
            p.isdft(c["dfts"], out=c["y"])
            expect(p, where)
            c.check({"y"}, what)
            return dict(outs=[G.to_numpy(c["y"])], state=p.state())

    def verify(res, where):
        what = (combo, N, n, latency, opts, tag(where))
        y = res["outs"][0]
        if exact:
            assert np.array_equal(y, want), (what, int((y != want).sum()))
            return
        for c in range(channels):
            dc, yc, wc = (d[c], y[c], want[c]) if channels > 1 else (d, y, want)
            yx, S = X.exact_synthesis(dc, N, latency)
            X.check_samples(X.sample_errors(yc, yx, S), X.sample_errors(wc, yx, S), X.synthesis_floor(combo, combo, N), what=what)

    base = run(None)
    verify(base, None)
    for where in (places if places is not None else placements({"dfts": fdx, "y": td}, wide="dfts")):
        got = run(where)
        verify(got, where)
        same_run(base, got, (combo, N, n, opts, tag(where)))


@pytest.mark.parametrize("combo,N,latency,rows", [("f32f32", 1000, 1.0, 4), ("f32f32", 1001, 0.5, 8), ("f64f32", 128, 1.0, 16), ("f32f32", 127, 0.5, 16),
                                                  ("f32f64", 1024, 0.5, 32), ("f64f64", 127, 1.0, 4), ("f32f64", 2048, 1.0, 16), ("f64f64", 1000, 0.5, 8)])
def test_synthesis_streaming_rows(combo, N, latency, rows):
    """The streaming kernel in the reference's order at 4 / 8 / 16 / 32 rows per wave (inverse_rows), rows that do not fill the last
    group, even and odd N at FD float -- where the 16-byte loads of an even N start 8 bytes past a 16-byte boundary on a
    misaligned matrix (sdft_inverse.hpp:574, :604)."""
    def expect(p, where):
        opt(p, last_inverse_form=1)
    synthesis_case(combo, N, 2100 + rows // 2 + 1, latency, dict(inverse_rows=rows), expect, seed=N)


@pytest.mark.parametrize("combo,N,latency", [("f32f32", 1000, 1.0), ("f64f32", 127, 0.5), ("f32f64", 1025, 0.5), ("f64f64", 128, 1.0), ("f32f32", 4096, 0.5)])
def test_synthesis_short_row_kernel(combo, N, latency):
    """Up to 1024 rows: one wave per row (inverse_row_kernel; vec_ok per row, sdft_inverse.hpp:693)."""
    def expect(p, where):
        opt(p, last_inverse_form=1)
    synthesis_case(combo, N, 333, latency, {}, expect, seed=N)


@pytest.mark.parametrize("N,latency", [(1000, 0.5), (1024, 1.0), (127, 1.0), (2050, 0.5)])
def test_synthesis_tree_sum_with_proof(N, latency):
    """Float samples from double bins, 1025 ... 8191 rows: the tree sum with the rounding-interval proof (form 2), the reference's bits."""
    def expect(p, where):
        opt(p, last_inverse_form=2)
    synthesis_case("f32f64", N, 2101, latency, {}, expect, seed=N)


@pytest.mark.parametrize("N", [1024, 1000, 64, 2048])
def test_synthesis_rows_in_step(N):
    def expect(p, where):
        opt(p, last_inverse_form=3)
    synthesis_case("f32f64", N, 2101, 1.0, dict(inverse_step=1), expect, seed=N)


@pytest.mark.parametrize("combo,N,latency", [("f32f32", 1000, 0.5), ("f32f32", 1024, 1.0), ("f64f32", 320, 1.0), ("f32f64", 1024, 0.5), ("f64f64", 1000, 1.0)])
def test_synthesis_ordered_rows_decline_a_misaligned_matrix(combo, N, latency):
    """inverse_ordered = 1: whole rows with the ordered sum (form 4) on an aligned matrix; a matrix 8 bytes past a 16-byte boundary
    must take another form (logic::rows_ordered_ok, 16-byte loads only) -- and give the same bits."""
    seen = set()

    def expect(p, where):
        form = p.get_option("last_inverse_form")
        if off16(where, "dfts"):
            assert form != 4, form
        else:
            assert form == 4, form
        seen.add(form == 4)
    synthesis_case(combo, N, 2101, latency, dict(inverse_ordered=1, inverse_tune=0), expect, seed=N)
    assert seen == ({True, False} if combo.endswith("f32") else {True})


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("N,latency", [(1000, 1.0), (127, 0.5), (4096, 0.5)])
def test_synthesis_unverified_tree_sum(combo, N, latency):
    """exact_inverse = 0 (form 0): per sample against the exact sum of the same rows (exact_sdft.check_samples)."""
    def expect(p, where):
        opt(p, last_inverse_form=0)
    synthesis_case(combo, N, 1300 if N < 4096 else 700, latency, dict(exact_inverse=0), expect, exact=False, seed=N)


@pytest.mark.parametrize("combo,N,opts", [("f32f32", 1000, dict(inverse_rows=4)), ("f32f64", 1024, dict(inverse_rows=16)), ("f32f64", 1000, dict(inverse_tune=0)),
                                          ("f64f32", 512, dict(inverse_rows=8))])
def test_synthesis_streaming_loads_of_both_kinds(combo, N, opts):
    """inverse_nt = 1 with inverse_nt_skip_mb = 3: the rows read first by ordinary loads, the rest by non-temporal loads, in one call."""
    def expect(p, where):
        opt(p, last_inverse_nt=1)
        assert p.get_option("last_inverse_skip") > 0
    synthesis_case(combo, N, 2101 if N > 512 else 4099, 0.5, dict(inverse_nt=1, inverse_nt_skip_mb=3, **opts), expect, seed=N)


def test_synthesis_batched_plan():
    def expect(p, where):
        opt(p, last_inverse_form=1)
    synthesis_case("f32f32", 96, 700, 0.5, dict(inverse_rows=4), expect, channels=3)


# ---- the fused call: sdft_hip_process_n ------------------------------------------------------------------------------------------
def process_case(combo, N, latency, op, lengths, opts, expect, exact, window="hann", with_dfts=False, in_place=False, device_gain=True,
                 host=False, seed=1, places=None):
    """Calls of `lengths` samples through the fused call.  exact: y against the two reference calls bit for bit (the hosts'
    operation as test_gpu_process.py states it); else per sample against the model (exact_sdft.check_pipeline), the copy of
    the spectrum per bin (check_bins).  Gain vectors travel as device buffers of the call (carved like the others)."""
    td, fd, fdx = O.combo_types(combo)
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    x = TE.signal(n, seed, td)
    kw = TE.op_kwargs(op, N, fd, fdx, rng)
    gain = kw.get("gain")
    starts = np.concatenate([[0], np.cumsum(lengths)])
    # the oracle's two calls, call by call (the rows of a time-varying gain count from the start of each call)
    ana, syn = O.best(N, window, 1.0, combo), O.best(N, window, latency, combo)
    d_ref = ana.sdft(x)
    y_ref, z_ref = [], []
    for i, n1 in enumerate(lengths):
        di = d_ref[starts[i]:starts[i + 1]]
        if op == "identity":
            zi = di
        elif op == "gain":
            zi = (di * gain[None, :].astype(fd)).astype(fdx)
        elif op in ("cgain", "cgain_rows", "gain_rows"):
            g = gain[None, :] if op == "cgain" else gain[np.minimum(np.arange(n1) // kw["hop"], gain.shape[0] - 1)]
            if op == "gain_rows":
                zi = (di * g.astype(fd)).astype(fdx)
            else:
                zi = np.empty_like(di)
                zi.real = di.real * g.real - di.imag * g.imag
                zi.imag = di.real * g.imag + di.imag * g.real
        elif op == "gate":
            mag2 = di.real * di.real + di.imag * di.imag
            thr2 = fd(kw["threshold"]) * fd(kw["threshold"])
            zi = np.where(mag2 < thr2, (di * np.where(mag2 < thr2, fd(kw["floor"]), fd(1))).astype(fdx), di)
        else:
            zi = TE.model_op(di, op, np.arange(n1), kw).astype(fdx)
        z_ref.append(zi)
        y_ref.append(syn.isdft(zi))

    def run(where):
        what = (combo, N, latency, op, opts, tag(where))
        with make(N, window, latency, combo, **opts) as p:
            bufs, dev, outs, geo = Buffers(where, host), Buffers(where, False), [], []
            for i, n1 in enumerate(lengths):
                part = x[starts[i]:starts[i + 1]]
                specs = [("x", (n1,), td, part)]
                if not in_place:
                    specs.append(("y", (n1,), td, None))
                side = []                                                   # device memory whatever the samples are
                if with_dfts:
                    side.append(("dfts", (n1, N), fdx, None))
                if gain is not None and device_gain:
                    side.append(("gain", gain.shape, gain.dtype, gain))
                if host:
                    b, c = bufs.call(specs), dev.call(side) if side else None
                else:
                    b = c = bufs.call(specs + side)                         # one arena for the whole call
                pkw = {k: v for k, v in kw.items() if k != "gain"}
                if gain is not None:
                    pkw["gain"] = c["gain"] if device_gain else gain
                y = b["x"] if in_place else b["y"]
                dd = c["dfts"] if with_dfts else None
                p.process(b["x"], op, out=y, dfts=dd, **pkw)
                expect(p, i, where)
                b.check({"x" if in_place else "y", "dfts"}, what + (i,))
                if c is not None and c is not b:
                    c.check({"dfts"}, what + (i, "device side"))
                outs.append(G.to_numpy(y))
                if with_dfts:
                    outs.append(G.to_numpy(dd))
                geo.append((p.get_option("last_chunks"), p.get_option("last_chunk_len")))
            return dict(outs=outs, state=p.state(), geo=geo)

    def verify(res, where):
        what = (combo, N, latency, op, opts, tag(where))
        step = 2 if with_dfts else 1
        ys = res["outs"][0::step]
        if exact:
            for i, y in enumerate(ys):
                assert np.array_equal(y, y_ref[i]), (what, "call", i, int((y != y_ref[i]).sum()))
            if not with_dfts:
                return
        J, Lc = max(g[0] for g in res["geo"]), max(g[1] for g in res["geo"])
        prng = np.random.default_rng(seed + 1)
        rows, tcall = [], []
        for i, n1 in enumerate(lengths):
            t0 = int(starts[i])
            r = sorted(TE.call_rows(N, t0, n1, res["geo"][i][1], res["geo"][i][0], prng) | {t0 + int(v) for v in prng.integers(0, n1, size=min(48, n1))})
            rows += r
            tcall += [t - t0 for t in r]
        rows, tcall = np.array(rows), np.array(tcall)
        call_of = np.searchsorted(starts, rows, side="right") - 1
        st = X.Stream(x, N, combo)
        A = st.A(rows)
        Zx = TE.model_op(st.rows(rows, window), op, tcall, kw)
        lip = TE.lipschitz(op, kw, A)
        B = X.serial_bound(combo, N, A, n) * lip
        keep = np.ones(rows.size, dtype=bool)
        if op == "gate":
            keep = X.gate_margin_ok(st.rows(rows, window), kw["threshold"], X.C_FACTOR * B)
            assert keep.sum() >= rows.size // 4, keep.sum()
        Zr = np.stack([z_ref[c][t] for c, t in zip(call_of, tcall)])
        if not exact:
            yx, S = X.exact_synthesis(Zx, N, latency)
            Fy = X.pipeline_floor(combo, combo, N, latency, S, B)
            yp = np.array([ys[c][t] for c, t in zip(call_of, tcall)])
            yr = np.array([y_ref[c][t] for c, t in zip(call_of, tcall)])
            X.check_pipeline(yp[keep], yr[keep], yx[keep], Fy[keep], what=what)
        if with_dfts:
            Zp = np.stack([res["outs"][1::2][c][t] for c, t in zip(call_of, tcall)])
            F = X.analysis_floor(combo, N, A, J, Lc) * lip
            X.check_bins(X.bin_errors(Zp[keep], Zx[keep]), X.bin_errors(Zr[keep], Zx[keep]), F, what=what + ("dfts",))

    if places is None:
        names = {"x": td}
        if not in_place: names["y"] = td
        if with_dfts: names["dfts"] = fdx
        if gain is not None and device_gain: names["gain"] = gain.dtype
        places = placements(names, wide="dfts" if with_dfts else None)
    base = run(None)
    verify(base, None)
    for where in places:
        got = run(where)
        verify(got, where)
        same_run(base, got, (combo, N, op, opts, tag(where)))


@pytest.mark.parametrize("combo,N,latency,op", [("f32f64", 1000, 0.5, "gain"), ("f32f32", 512, 1.0, "cgain"), ("f64f64", 1024, 1.0, "identity"),
                                                ("f64f32", 4096, 0.5, "gain_rows"), ("f32f64", 2048, 1.0, "cgain_rows")])
def test_fused_folded_form(combo, N, latency, op):
    """fused_exact = 0, fold = 1 (fold_coeff_kernel + process_rows_kernel), then a hop through the folded hop kernel: per sample
    against the model.  Gain vectors are device buffers at odd element offsets."""
    def expect(p, i, where):
        if i == 1 and op.endswith("_rows"):
            opt(p, last_process_path=2, last_chunks=1)                         # (a hop with gains that change in time: hop kernel + row synthesis)
            return
        opt(p, last_process_path=1, last_fused_fold=1)
        if i == 0: opt(p, last_fused_exact=0)
        assert (p.get_option("last_chunks") > 1) == (i == 0)
    process_case(combo, N, latency, op, [2 * N + 1501, 100], dict(fused_exact=0), expect, False, seed=N)


@pytest.mark.parametrize("combo,N,op,opts", [("f32f64", 1024, "gain", dict(fold=0)), ("f32f32", 2048, "cgain", dict(fold=0)), ("f32f64", 1000, "gate", {}),
                                             ("f32f32", 512, "expr", {}), ("f64f64", 1500, "identity", dict(fold=0)), ("f32f32", 3000, "gain", dict(fold=0))])
def test_fused_windowed_rows_with_a_copy_of_the_spectrum(combo, N, op, opts):
    """fold = 0: the windowed rows stay in LDS (two slots per lane at N = 1500 double / 3000 float), the operation runs on them, and
    the processed spectrum is copied out into a guarded dfts -- its stores are the row-group kernel's (vec_store on q.out = dfts)."""
    def expect(p, i, where):
        opt(p, last_process_path=1, last_fused_fold=0)
    process_case(combo, N, 0.5, op, [2 * N + 1203], dict(fused_exact=0, **opts), expect, False, window="blackman", with_dfts=True, seed=N)


@pytest.mark.parametrize("combo,N,op,opts,path", [("f32f32", 512, "cgain", dict(fused_exact=1), 1), ("f64f32", 1000, "gain", dict(fused_exact=1), 1),
                                                  ("f32f64", 1024, "identity", dict(carry=1, fused_exact=2), 1), ("f64f64", 256, "gain", dict(carry=1), 1),
                                                  ("f32f32", 4096, "gain", dict(fused_exact=2), 1), ("f32f32", 4096, "identity", dict(fused_exact=1), 3),
                                                  ("f32f32", 512, "gain_rows", dict(fused_exact=1), 1), ("f32f32", 512, "gate", dict(fused_exact=1), 1)])
def test_fused_reference_order_is_bit_identical(combo, N, op, opts, path):
    """fused_exact = 1 / 2 (and carry = 1 at FD double): the two reference calls bit for bit, through the fused kernel (path 1) or,
    for two-slot rows at FD float with fused_exact = 1, the two passes (3)."""
    def expect(p, i, where):
        opt(p, last_process_path=path)
        if path == 1: opt(p, last_fused_exact=1)
    process_case(combo, N, 1.0 if N != 1000 else 0.5, op, [1900 + N // 4], opts, expect, True, seed=N)


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("op", ["cgain", "identity"])
def test_fused_hop_pair_is_bit_identical(combo, op):
    """Calls of one time chunk with fused_exact = 1: hop kernel + one-wave-per-row synthesis (path 2), bit-identical."""
    def expect(p, i, where):
        opt(p, last_process_path=2, last_chunks=1)
    process_case(combo, 1000, 1.0, op, [100, 100, 37], dict(fused_exact=1), expect, True, seed=11)


@pytest.mark.parametrize("op", ["identity", "gate"])
def test_fused_two_pass_path(op):
    """N = 5000: rows beyond every fused kernel -- analysis and synthesis through the plan's workspace (path 3)."""
    def expect(p, i, where):
        opt(p, last_process_path=3)
    process_case("f32f64", 5000, 0.5, op, [2 * 5000 + 701], {}, expect, False, seed=4)


@pytest.mark.parametrize("combo,N,n,opts,exact", [("f32f64", 1024, 9000, {}, False), ("f32f64", 256, 100, dict(fused_exact=1), True),
                                                  ("f32f32", 512, 5000, dict(fused_exact=1), True), ("f64f64", 1000, 3000, {}, False)])
def test_fused_in_place_inside_the_arena(combo, N, n, opts, exact):
    """out == samples: the library copies the samples aside; nothing but the n samples of the one buffer is written."""
    def expect(p, i, where):
        opt(p, last_process_path=(1, 2))
    process_case(combo, N, 1.0, "gain", [n], opts, expect, exact, in_place=True, seed=N)


# ---- row-pointer variants and single-sample calls (sdft_amd.capi.Api) --------------------------------------------------------------
@pytest.mark.parametrize("combo,N", [("f32f32", 100), ("f64f32", 128), ("f32f64", 100)])
@pytest.mark.parametrize("table_on_device", [False, True])
def test_row_pointer_variants_with_rows_carved_one_by_one(combo, N, table_on_device):
    """sdft_sdft_nd / sdft_isdft_nd: every row its own guarded view, at FD float alternating between 0 and 8 bytes past a 16-byte
    boundary (the row kernel's vec_ok is per row); the pointer table on the host and on the device; a hop (last_kernel 3) and a
    call of several chunks (independent tiles: 1)."""
    import torch
    from sdft_amd.capi import Api
    td, fd, fdx = O.combo_types(combo)
    api = Api(combo)
    lengths = [64, 600]
    x = TE.signal(sum(lengths), 8, td)
    ref = O.best(N, "blackman", 0.5, combo)
    res = {}
    for guarded in (False, True):
        plan = api.alloc_custom(N, 3, 0.5)
        assert plan and api.set_option(plan, b"carry", 1) == 0              # (bit-identical at FD double too)
        t0, outs = 0, []
        for n in lengths:
            part = np.ascontiguousarray(x[t0:t0 + n])
            if guarded:
                arena = G.DeviceArena(n * (N * np.dtype(fdx).itemsize + 2 * G.MIN_GUARD + 512) + 512)
                rows = [arena.carve((N,), fdx, 8 * (i % 2) if fd == np.float32 else 0, name=f"row{i}") for i in range(n)]
                host = G.HostArena(G.room(((n,), td), ((n,), td), ((n,), np.uint64)))
                xv = G.put(host.carve((n,), td, np.dtype(td).itemsize, name="x"), part)
                y = host.carve((n,), td, np.dtype(td).itemsize, name="y")
                table = host.carve((n,), np.uint64, 8, name="table")
            else:
                rows = [torch.empty(N, dtype=getattr(torch, np.dtype(fdx).name), device="cuda") for _ in range(n)]
                xv, y, table = part, np.empty(n, dtype=td), np.empty(n, dtype=np.uint64)
            table[:] = [r.data_ptr() for r in rows]
            if table_on_device:
                tdev = torch.from_numpy(np.array(table).view(np.int64)).cuda()
                tptr = C.c_void_p(tdev.data_ptr())
            else:
                tptr = C.c_void_p(table.ctypes.data)
            api.clear()
            api.sdft_nd(plan, n, C.c_void_p(xv.ctypes.data), tptr)
            api.check()
            assert api.get_option(plan, b"last_kernel") == (3 if n < 512 else 1), api.get_option(plan, b"last_kernel")
            got = torch.stack(rows).cpu().numpy()
            api.isdft_nd(plan, n, tptr, C.c_void_p(y.ctypes.data))
            api.check()
            torch.cuda.synchronize()
            if guarded:
                arena.check(); host.check()
                assert all(G.view_unwritten(r) == 0 for r in rows[:: max(1, n // 40)]) and G.view_unwritten(y) == 0
                assert same_bits(np.array(xv), part)
            want = ref.sdft(part) if not guarded else res[False][len(outs)]
            if not guarded:
                assert np.array_equal(got, want), (combo, N, n)                              # (exact carries or one chunk)
                assert np.array_equal(y, O.best(N, "blackman", 0.5, combo).isdft(want)), (combo, N, n)
            outs += [got, np.array(y)]
            t0 += n
        api.free(plan)
        res[guarded] = outs
    for a, b in zip(res[False], res[True]):
        assert same_bits(a, b)


@pytest.mark.parametrize("combo", ["f32f32", "f64f32", "f32f64", "f64f64"])
@pytest.mark.parametrize("resident", [0, 1])
def test_single_sample_calls_on_a_guarded_row(combo, resident):
    """sdft_sdft / sdft_isdft on a device row carved from an arena (FD float: 8 bytes past a 16-byte boundary as well; FD double: 16
    bytes past a 128-byte boundary), through the launches and through the resident kernel, across the roll-over."""
    import torch
    from sdft_amd.sdft import SDFT
    td, fd, fdx = O.combo_types(combo)
    N, n = 96, 2 * 96 + 37
    x = TE.signal(n, 4, td)
    ref = O.best(N, "hamming", 1.0, combo)
    want = ref.sdft(x); ywant = ref.isdft(want)
    res = {}
    for where in [None, 0] + list(residues(fdx)) + [(16, 128)]:
        with SDFT(N, "hamming", 1.0, combo) as p:
            p.set_option("resident", resident)
            arena = None
            if where is None:
                row = torch.empty(N, dtype=getattr(torch, np.dtype(fdx).name), device="cuda")
            else:
                arena = G.DeviceArena(G.room(((N,), fdx)))
                row = arena.carve((N,), fdx, *(where if isinstance(where, tuple) else (where, 16)), name="row")
            rows, ys = [], []
            for i in range(n):
                p.api.sdft(p._p, td(x[i]).item(), C.c_void_p(row.data_ptr()))
                ys.append(p.api.isdft(p._p, C.c_void_p(row.data_ptr())))
                if i % 16 == 0 or i >= 2 * N - 2:
                    rows.append(row.cpu().numpy().copy())
                    assert np.array_equal(rows[-1], want[i]), (combo, resident, where, i)
                    if arena is not None:
                        arena.check()
            p.api.check()
            opt(p, last_kernel=3)
            if resident:
                assert p.get_option("resident_calls") >= 2 * n - 4 * len(rows) - 4, (p.get_option("resident_calls"), n)
            else:
                opt(p, resident_calls=0)
            assert np.array_equal(np.array(ys, dtype=td), ywant), (combo, resident, where)
            res[where] = dict(outs=rows + [np.array(ys, dtype=td)], state=p.state())
            state_is_the_oracles(res[where]["state"], [ref], (combo, resident, where))
        if where is not None:
            same_run(res[None], res[where], (combo, resident, where))


# ---- host pointers ------------------------------------------------------------------------------------------------------------------
HOST_OPTIONS = [{}, dict(pinned_io=0), dict(copy_threads=0), dict(stage_bytes=1 << 20), dict(host_register=1)]


def host_places(bufs):
    """Host views at odd element offsets: every buffer one element past a 16-byte boundary, and everything at its largest residue."""
    one = {name: np.dtype(dt).itemsize % 16 for name, dt in bufs.items()}
    return [one, {name: (max(residues(dt)) if residues(dt) else (80, 128)) for name, dt in bufs.items()}]


@pytest.mark.parametrize("opts", HOST_OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
@pytest.mark.parametrize("combo", ["f32f32", "f64f64"])
def test_host_pointers_analysis_and_synthesis(combo, opts):
    """sdft_sdft_n / sdft_hip_sdft_every_n / sdft_isdft_n on HostArena views at odd element offsets, through the staging path (several
    segments with stage_bytes = 1 MiB), the pinned scratch (a hop's samples), the calling thread alone, and buffers registered in
    place (host_register: the matrices here are larger than 1 MiB and live as long as the plan).  host_copy stays 0."""
    td, fd, fdx = O.combo_types(combo)
    N = 256
    exact = dict(carry=1) if combo.endswith("f64") else {}
    hits = []

    def expect(p, i, where):
        opt(p, host_copy=0)
        if i == 0 and "host_register" in opts:
            hits.append(p.get_option("host_register_hits") + p.get_option("host_register_misses"))
    analysis_case(combo, N, [3000, 100, 700], dict(exact, **opts), expect, True, host=True, places=host_places({"x": td, "out": fdx}), seed=6)
    if "host_register" in opts:
        assert all(h > 0 for h in hits), hits
    analysis_case(combo, N, [3000, 300], dict(exact, **opts), lambda p, i, where: opt(p, last_kernel=4), True, host=True, every=100, first=42,
                  places=host_places({"x": td, "out": fdx}), seed=7)
    for n in (3000, 100):
        synthesis_case(combo, N, n, 0.5, dict(opts), lambda p, where: opt(p, host_copy=0), host=True, places=host_places({"dfts": fdx, "y": td}), seed=n)


@pytest.mark.parametrize("opts", HOST_OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_host_pointers_fused_call(opts):
    """sdft_hip_process_n with host samples (and a device dfts in the guarded run's own device arena): a long call and a hop."""
    def expect(p, i, where):
        opt(p, host_copy=0, last_process_path=(1, 2))
    places = host_places({"x": np.float32, "y": np.float32})
    process_case("f32f32", 512, 1.0, "gain", [20000, 100], dict(fused_exact=1, **opts), expect, True, host=True, places=places, seed=8)
    process_case("f32f64", 1024, 0.5, "cgain", [3000], dict(fused_exact=0, fold=0, **opts), lambda p, i, where: opt(p, last_process_path=1), False, host=True,
                 with_dfts=True, places=[dict(w, dfts=(16, 128)) for w in places], seed=9)
