"""The prefix-cell route of long analysis calls: one pre-pass launch (prefix_cells_kernel) writes, for every chunk, the 2N cells
the self-carried form would fold for itself; the row-group kernel reads them and goes on as a self-carried chunk.

The additions of a cell are made in time order into one accumulator, so the cells -- and with them every row and the state --
are BIT-IDENTICAL to the self-carried route at the same chunk length.  That identity is the test; beside it the bars the
existing chunk-parallel tests hold: 1e-11 against the oracle, 1e-12 against the pre-pass of partial sums + scan.

The route is forced on short calls by the test hook prefix_cells = 2 with a forced chunk length.  Shapes are the smallest at
which each part of the kernel can go wrong (see CASES)."""

import numpy as np
import pytest

import exact_sdft as X
import guarded as G
from oracle import oracle as O
from sdft_amd.signals import noise

pytestmark = pytest.mark.gpu


def make(N, window="hann", combo="f32f64", channels=1, **opts):
    from sdft_amd.sdft import SDFT
    p = SDFT(N, window, 1.0, combo, channels)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    scale = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / scale if scale else float(np.abs(a).max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint64), b.reshape(-1).view(np.uint64))


def took_prefix(p):
    assert p.get_option("last_prefix") == 1 and p.get_option("last_self") == 0 and p.get_option("last_kernel") == 2, \
        (p.get_option("last_prefix"), p.get_option("last_self"), p.get_option("last_kernel"))


# (what it exercises, m, the two calls, chunk)
CASES = [
    ("chunks shorter than 2N, ragged last chunk, second call from cursor != 0 across the roll-over", 64, (3 * 128 + 517, 777), 40),
    ("chunk = 2N", 64, (5 * 128 + 3, 640), 128),
    ("chunks longer than 2N: two samples of a cell inside one chunk", 64, (1500, 1111), 136),
    ("first call shorter than 2N: the delay line feeds every old sample", 512, (600, 2100), 200),
    ("mixed-radix cells, 2N = 200", 100, (2 * 200 + 1503, 999), 192),
    ("mixed-radix cells, 2N = 2000", 1000, (2 * 2000 + 1503, 999), 192),
    ("smallest row group", 8, (2000, 513), 72),
    ("the headline's geometry in small", 1024, (9000, 5000), 1960),
    ("more than 512 rows per cell: the kernel's outer loop carries the running sums from one block of 512 rows to the next (3 blocks, then 2)", 8, (17000, 9001), 520),
]
RUNS = [("f32f64", i, "hann", 1) for i in range(len(CASES))] + [("f64f64", i, "hann", 1) for i in (0, 1, 2, 8)] + \
       [("f32f64", 0, "hann", 3), ("f32f64", 2, "blackman", 1), ("f32f64", 4, "boxcar", 1)]


def three_routes(combo, m, lengths, chunk, window, channels, seed):
    """The calls on three plans: prefix cells, self-carried chunks, pre-pass.  Returns per call (prefix, self, prepass) matrices,
    the states of the first two plans and the samples."""
    import torch
    td, fd, fdx = O.combo_types(combo)
    xs = [np.stack([noise(n, seed=seed + 7 * i + 101 * c, dtype=td) for c in range(channels)]) for i, n in enumerate(lengths)]
    if channels == 1:
        xs = [x[0] for x in xs]
    outs = []
    with make(m, window, combo, channels, chunk=chunk, carry=0, prefix_cells=2) as p, \
         make(m, window, combo, channels, chunk=chunk, carry=0, prefix_cells=0, self_carry=1) as q, \
         make(m, window, combo, channels, chunk=chunk, carry=0, self_carry=0) as old:
        for x in xs:
            xd = torch.from_numpy(x).cuda()
            a = p.sdft(xd).cpu().numpy()
            took_prefix(p)                                                                    # (a)
            assert p.get_option("last_chunk_len") == chunk and p.get_option("last_chunks") == -(-len(x.T) // chunk)
            b = q.sdft(xd).cpu().numpy()
            assert q.get_option("last_self") == 1 and q.get_option("last_prefix") == 0 and q.get_option("last_chunk_len") == chunk
            c = old.sdft(xd).cpu().numpy()
            assert old.get_option("last_self") == 0 and old.get_option("last_prefix") == 0 and old.get_option("last_chunks") > 1
            outs.append((a, b, c))
        return outs, p.state(), q.state(), xs


@pytest.mark.parametrize("combo,case,window,channels", RUNS)
def test_prefix_cells_route(combo, case, window, channels):
    what, m, lengths, chunk = CASES[case]
    outs, sp, sq, xs = three_routes(combo, m, lengths, chunk, window, channels, seed=300 + case)
    refs = [O.best(m, window, 1.0, combo) for _ in range(channels)]
    for i, (a, b, c) in enumerate(outs):
        assert same_bits(a, b), (what, "call", i, "rows differ from the self-carried route", int((a != b).sum()))      # (b)
        for ch in range(channels):
            want = refs[ch].sdft(xs[i][ch] if channels > 1 else xs[i])
            got, pre = (a[ch], c[ch]) if channels > 1 else (a, c)
            e_ref, e_old = rel_err(got, want), rel_err(got, pre)
            print(f"PREFIX {combo} m={m} {window} call {i} channel {ch}: oracle {e_ref:.3g}  pre-pass {e_old:.3g}")
            assert e_ref <= 1e-11, (what, i, ch, e_ref)                                                                 # (c)
            assert e_old <= 1e-12, (what, i, ch, e_old)                                                                 # (d)
    for name, u, v in zip(("acc", "fid", "hist"), sp[:3], sq[:3]):
        assert same_bits(u, v) if u.dtype.itemsize % 8 == 0 else np.array_equal(u.view(np.uint32), v.view(np.uint32)), (what, "state", name)
    assert sp[3] == sq[3] == sum(lengths) % (2 * m)


def test_prefix_cells_into_guarded_misaligned_buffers():
    """(e) samples 4 bytes past a 16-byte boundary, the matrix 16 bytes past a 256-byte boundary, NaN guards on every side: guards
    intact, every row written, rows equal to the unguarded run bit for bit."""
    what, m, lengths, chunk = CASES[0]
    td, fd, fdx = O.combo_types("f32f64")
    import torch
    xs = [noise(n, seed=300 + 7 * i, dtype=td) for i, n in enumerate(lengths)]
    with make(m, "hann", "f32f64", 1, chunk=chunk, carry=0, prefix_cells=2) as base, \
         make(m, "hann", "f32f64", 1, chunk=chunk, carry=0, prefix_cells=2) as p:
        for i, x in enumerate(xs):
            want = base.sdft(torch.from_numpy(x).cuda()).cpu().numpy()
            arena = G.DeviceArena(G.room(((len(x),), td), ((len(x), m), fdx)))
            xv = G.put(arena.carve((len(x),), td, 4, 16, name="x"), x)
            ov = arena.carve((len(x), m), fdx, 16, 256, name="out")
            p.sdft(xv, out=ov)
            took_prefix(p)
            arena.check()
            assert G.view_unwritten(ov) == 0
            assert np.array_equal(G.to_numpy(xv).view(np.uint32), x.view(np.uint32))
            assert same_bits(G.to_numpy(ov), want), (what, "call", i)
        for u, v in zip(base.state()[:2], p.state()[:2]):
            assert same_bits(u, v)


def test_product_plan_takes_the_route_beyond_half_a_million_samples():
    """(f) no hook: n = 2^19 + 4096 takes the prefix cells, n = 2^19 the self-carried chunks; sampled rows against the oracle."""
    import torch
    from test_gpu_exact import call_rows
    m, combo = 64, "f32f64"
    n = (1 << 19) + 4096
    x = noise(n, seed=77)
    with make(m, "hann", combo) as p:
        out = torch.empty((n, m), dtype=torch.complex128, device="cuda")
        xd = torch.from_numpy(x).cuda()
        p.sdft(xd, out=out)
        assert not p.api.hooks
        took_prefix(p)
        rng = np.random.default_rng(77)
        rows = np.array(sorted(call_rows(m, 0, n, p.get_option("last_chunk_len"), p.get_option("last_chunks"), rng)))
        got = out.index_select(0, torch.tensor(rows, device="cuda")).cpu().numpy()
        want = X.oracle_rows(O.best(m, "hann", 1.0, combo), x, rows, chunk=1 << 16)
        e = rel_err(got, want)
        print(f"PREFIX product plan n={n}: oracle {e:.3g} on {len(rows)} rows")
        assert e <= 1e-11, e
        p.reset()
        p.sdft(xd[:1 << 19], out=out[:1 << 19])
        assert p.get_option("last_self") == 1 and p.get_option("last_prefix") == 0 and not p.api.hooks


def test_product_plan_keeps_the_partial_sums_beyond_the_bound_of_rows_per_cell():
    """No hook: m = 8 at n = 2^19 + 4096 is 33 024 rows per cell on one workgroup, beyond logic::kPrefixRowsMax: partial sums + scan,
    as before the route existed; sampled rows against the oracle."""
    import torch
    from test_gpu_exact import call_rows
    m, combo = 8, "f32f64"
    n = (1 << 19) + 4096
    x = noise(n, seed=78)
    with make(m, "hann", combo) as p:
        out = torch.empty((n, m), dtype=torch.complex128, device="cuda")
        p.sdft(torch.from_numpy(x).cuda(), out=out)
        assert not p.api.hooks
        assert p.get_option("last_prefix") == 0 and p.get_option("last_self") == 0 and p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 2
        rng = np.random.default_rng(78)
        rows = np.array(sorted(call_rows(m, 0, n, p.get_option("last_chunk_len"), p.get_option("last_chunks"), rng)))
        got = out.index_select(0, torch.tensor(rows, device="cuda")).cpu().numpy()
        want = X.oracle_rows(O.best(m, "hann", 1.0, combo), x, rows, chunk=1 << 16)
        e = rel_err(got, want)
        print(f"PREFIX product plan beyond the bound n={n} m={m}: oracle {e:.3g} on {len(rows)} rows")
        assert e <= 1e-11, e
