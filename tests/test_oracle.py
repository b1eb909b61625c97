"""The oracle itself: pinned against the genuine reference build (when present in this
container) and against the committed golden vectors that build produced."""

import glob
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from sdft_amd.signals import noise, sine_sweep

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def digest_of(d, block=4096):
    """per-row checksums (sum re, sum im, sum |.|^2, sum (k+1) re), computed in row blocks to keep the
    temporaries small"""
    k = np.arange(1, d.shape[1] + 1, dtype=np.float64)
    out = np.empty((d.shape[0], 4), dtype=np.float64)
    for i in range(0, d.shape[0], block):
        re = d[i:i + block].real.astype(np.float64); im = d[i:i + block].imag.astype(np.float64)
        out[i:i + block] = np.stack([re.sum(1), im.sum(1), (re * re + im * im).sum(1), (re * k).sum(1)], axis=1)
    return out


def test_port_matches_tiny_golden_cases_bit_for_bit():
    z = load("tiny_cases.npz")
    keys = sorted({k.rsplit("/", 1)[0] for k in z})
    assert len(keys) == 240
    for key in keys:
        combo, window, lat, m = key.split("/")
        p = O.Port(int(m), window, int(lat) / 100.0, combo)
        d = p.sdft(z[key + "/x"])
        assert np.array_equal(d, z[key + "/d"]), key
        assert np.array_equal(p.isdft(d), z[key + "/y"]), key


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "mid_*.npz")) + glob.glob(os.path.join(GOLD, "cfg*.npz"))))
def test_port_matches_golden_fixture(path):
    g = load(os.path.basename(path))
    m, window, latency, combo = int(g["dftsize"]), str(g["window"]), float(g["latency"]), str(g["combo"])
    p = O.Port(m, window, latency, combo)
    x = g["x"]
    # stream in hops (the fixture's own hop, or 4096 rows) through one reused buffer: the state
    # persists across calls, and the test never touches a 786 MB matrix (first-touch page faults
    # dominate the runtime in a sandbox)
    hop = int(g["hop"]) if "hop" in g else 4096
    buf = np.empty((hop, m), dtype=O.combo_types(combo)[2])
    wanted = {int(t): i for i, t in enumerate(g["rows_idx"])}
    ys = []
    for t0 in range(0, x.size, hop):
        cnt = min(hop, x.size - t0)
        d = p.sdft(x[t0:t0 + cnt], buf[:cnt])
        assert np.array_equal(digest_of(d), g["digest"][t0:t0 + cnt])
        for t in range(t0, t0 + cnt):
            if t in wanted:
                assert np.array_equal(d[t - t0], g["rows"][wanted[t]]), t
        ys.append(p.isdft(d))
    assert np.array_equal(np.concatenate(ys), g["y"])


def test_port_matches_reference_test_wav_fixture():
    """The reference's own end-to-end test shape: test.wav, m=1000, hop=100, Hann (test/main.sh:3-6)."""
    g = load("testwav_m1000_hop100_hann_f32f64.npz")
    p = O.Port(1000, "hann", 1.0, "f32f64")
    hop = int(g["hop"])
    x = g["x"]
    firsts, ys = [], []
    for i in range(0, x.size, hop):
        d = p.sdft(x[i:i + hop])
        firsts.append(d[0]); ys.append(p.isdft(d))
    assert np.array_equal(np.stack(firsts), g["hop_first_rows"])
    assert np.array_equal(np.concatenate(ys), g["y"])


def test_digest_streaming_equals_matrix():
    x = sine_sweep(3000)
    a = O.Port(128, "hann"); b = O.Port(128, "hann")
    d = a.sdft(x)
    dig, y = b.digest(x)
    # the C digest sums serially in bin order, numpy pairwise: equal up to summation rounding
    assert np.allclose(dig, digest_of(d), rtol=1e-12, atol=1e-13)
    assert np.array_equal(y, a.isdft(d))


def test_roundtrip_latency_and_snr():
    """Synthesis returns the input delayed by (N-1)*latency samples
    (/root/reference/python/examples/latency.py:30); the SNR depends on the signal (about 23 dB
    for white noise, about 60 dB for the sweep with a Hann window at latency 1)."""
    m = 256
    for x, floor in ((noise(8 * m), 20.0), (sine_sweep(8 * m), 50.0)):
        p = O.Port(m, "hann", 1.0)
        y = p.isdft(p.sdft(x)).astype(np.float64)
        x = x.astype(np.float64)
        snr = {}
        for lag in range(m - 4, m + 3):
            err = y[2 * m + lag:] - x[2 * m:-lag]
            snr[lag] = 10 * np.log10(np.mean(x[2 * m:-lag] ** 2) / np.mean(err ** 2))
        assert max(snr, key=snr.get) == m - 1
        assert snr[m - 1] > floor


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("combo", O.COMBOS)
def test_port_equals_reference_build(combo):
    """Tables, rows and samples of ragged hops across the roll-over, the state, and a call after reset(): the port's bits are
    the reference's -- checked against the digests the reference build produced (tests/golden/port_vs_reference.json), and
    against the reference build itself, array for array, where oracle/_ref is present."""
    g = _make_golden()
    with open(os.path.join(GOLD, "port_vs_reference.json")) as fh:
        stored = json.load(fh)[combo]
    assert len(stored) == len(g.TRACE_CASES)
    for m, window, latency in g.TRACE_CASES:
        mine = g.trace(O.Port(m, window, latency, combo), combo, m)
        assert g.trace_digests(mine) == stored[f"{m}/{window}/{latency}"], (combo, m, window, latency)
        if O.have_reference(combo):
            theirs = g.trace(O.Reference(m, window, latency, combo), combo, m)
            assert len(mine) == len(theirs)
            for a, b in zip(mine, theirs):
                assert np.array_equal(a, b), (combo, m, window, latency)
