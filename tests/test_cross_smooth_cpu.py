"""Smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n) without a GPU: the symbol of every type pair, the NULL-plan
error, the coherence helper on a hand example, the refusals SDFT.cross_smooth makes before it touches a plan, the declarations in
the headers, the host-side logic (kernel id, route and time chunks, unit row, workspace and slots with pairs for channels, the
decay check, the chunked scheme on signed terms against the sequential loop; tests/cpp/cross_smooth_logic_test.cpp under g++
-fsanitize=address,undefined) and the kernel's instantiations in every translation unit's gfx950 code object -- without atomics,
LDS, scratch or a fused multiply-add on the value path, and with the two carry kernels of the smoothed power call as they were."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")


def test_cross_smooth_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_cross_smooth_n_{combo}"), combo
        assert "sdft_cross_smooth_n" in capi.typed_signatures(combo)
        assert capi.typed_signatures(combo)["sdft_cross_smooth_n"] == capi.typed_signatures(combo)["sdft_power_smooth_n"]


@pytest.mark.parametrize("combo", COMBOS)
def test_cross_smooth_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    for decay in (0.5, float("nan")):
        assert api.sdft_cross_smooth_n(None, 100, None, 10, 0, 0, 1, decay, None, None) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_cross_smooth_n" in err and "NULL plan" in err, err
        api.clear()


def test_coherence_on_a_hand_example():
    from sdft_amd.sdft import coherence
    s_ab = np.array([[3 + 4j, 0j, 1 + 1j, 2j], [1 + 0j, -6 + 8j, 0j, 5 + 0j]])
    s_aa = np.array([[5.0, 2.0, 4.0, 0.0], [1.0, 10.0, 3.0, 10.0]])
    s_bb = np.array([[5.0, 3.0, 1.0, 7.0], [4.0, 10.0, 2.0, 5.0]])
    want = np.array([[1.0, 0.0, 0.5, np.nan], [0.25, 1.0, 0.0, 0.5]])
    got = coherence(s_ab, s_aa, s_bb)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
    # the auto-spectra as cross_smooth returns them -- complex, imaginary part 0 -- and single precision in
    got = coherence(s_ab.astype(np.complex64), s_aa.astype(np.complex64), (s_bb + 0j).astype(np.complex64))
    assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
    # a channel against itself
    z = np.array([2.5 + 0j, 1e-3 + 0j])
    assert np.array_equal(coherence(z, z, z), [1.0, 1.0])
    # broadcasting over rows
    assert coherence(s_ab, s_aa[0], s_bb[0]).shape == (2, 4)


def test_cross_smooth_refusals_of_the_python_call_before_a_plan_is_touched(hip_library):
    """a bad grid, band or decay, a plan without pairs and a state that cannot be updated in place are refused by
    SDFT.cross_smooth itself (the C call's own refusals need a plan, hence a GPU: tests/test_gpu_cross_smooth.py)"""
    from sdft_amd import sdft as S

    class NoPlan:
        dftsize = 8
        channels = 2
        fd = np.float32
        fdx = np.complex64
        pairs = 3

        class api:
            @staticmethod
            def clear():
                pass

    class NoPairs(NoPlan):
        pairs = 0

    x = np.zeros((2, 4), dtype=np.float32)
    for bad in (float("nan"), -0.25, 1.0, 1.0 - 2.0 ** -26, 7):
        with pytest.raises(ValueError, match="decay"):
            S.SDFT.cross_smooth(NoPlan(), x, bad)
    with pytest.raises(ValueError):
        S.SDFT.cross_smooth(NoPlan(), x, 0.5, every=0)
    for bins in ((0, 0), (8, 1), (1, 8)):
        with pytest.raises(ValueError):
            S.SDFT.cross_smooth(NoPlan(), x, 0.5, bins=bins)
    with pytest.raises(ValueError, match="set_pairs"):
        S.SDFT.cross_smooth(NoPairs(), x, 0.5)
    for state in (np.zeros((3, 8), dtype=np.complex128), np.zeros((3, 8), dtype=np.float32), np.zeros((3, 7), dtype=np.complex64),
                  np.zeros((2, 8), dtype=np.complex64), np.zeros(24, dtype=np.complex64), np.zeros((3, 16), dtype=np.complex64)[:, ::2], [[0j] * 8] * 3):
        with pytest.raises(ValueError, match="state"):
            S.SDFT.cross_smooth(NoPlan(), x, 0.5, state=state)
    frozen = np.zeros((3, 8), dtype=np.complex64)
    frozen.setflags(write=False)
    with pytest.raises(ValueError, match="state"):
        S.SDFT.cross_smooth(NoPlan(), x, 0.5, state=frozen)


def test_cross_smooth_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    assert "sdft_hip_sdft_cross_smooth_n(" in c_header and "SDFT_HIP_SYMBOL(sdft_cross_smooth_n)" in c_header
    assert "const double decay, sdft_fdx_t* state, sdft_fdx_t* smooth)" in c_header
    assert '("last_kernel" = 16)' in c_header and "16 (smoothed cross-spectrum analysis)" in c_header
    assert "8 u M / (1 - a)" in c_header and "m[t] = a * m[t-1] + b * |term[t]|" in c_header
    assert "sdft_hip_sdft_cross_smooth_n_##SUF" in cpp_header and "std::size_t cross_smooth(" in cpp_header


def test_cross_smooth_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "cross_smooth_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "cross_smooth_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    print(r.stdout)
    assert "cross-smooth-logic: all properties hold" in r.stdout
    ratios = [float(v) for v in re.findall(r"largest chunked error on signed terms ([0-9.]+) u M", r.stdout)]
    assert len(ratios) == 2 and all(v <= 8.0 for v in ratios), r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_cross_smooth_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_cross_smooth_kernel at the type pair's one bins-per-lane are in the translation
    unit's gfx950 code object; none of them holds an atomic, an LDS access or a scratch access, and the term and the recursion
    have no fused multiply-add of the FD type.  The cross-spectrum and smoothed power kernels beside them, and the two carry
    kernels the call launches as they are, are the sets they were."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_cross_smooth_kernel")}
    assert found == {f"forward_cross_smooth_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(found)
    fused = r"v_fma(c|mk|ak)?_f64|v_pk_fma" if fd == "double" else r"v_pk_fma|v_fma_f64"
    for name in found:
        ops = [line.split()[0] for line in kernels[name] if line]
        assert not [o for o in ops if "atomic" in o], name
        assert not [o for o in ops if o.startswith(("ds_", "scratch_"))], name
        assert not [o for o in ops if re.match(fused, o)], name
    helpers = {name for name in kernels if name.startswith(("smooth_scan_kernel", "smooth_fix_kernel"))}
    assert helpers == {f"smooth_scan_kernel<{fd}>", f"smooth_fix_kernel<{fd}>"}, sorted(helpers)
    cross = {name for name in kernels if name.startswith("forward_cross_sum_kernel")}
    assert cross == {f"forward_cross_sum_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(cross)
    smooth = {name for name in kernels if name.startswith("forward_power_smooth_kernel")}
    assert smooth == {f"forward_power_smooth_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(smooth)
