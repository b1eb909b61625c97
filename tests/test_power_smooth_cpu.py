"""Smoothed power analysis (sdft_hip_sdft_power_smooth_n) without a GPU: the symbol of every type pair, the NULL-plan error, the
Python helpers (smooth_coefficients, smooth_decay) and the refusals SDFT.power_smooth makes before it touches a plan, the
declarations in the headers, the host-side logic (kernel id, route and time chunks, rows, workspace and slots, the decay check,
the table of the decay's powers, the fix-up's chunk-and-offset rule, the chunked scheme against the sequential loop;
tests/cpp/power_smooth_logic_test.cpp under g++ -fsanitize=address,undefined) and the kernels' instantiations in every translation
unit's gfx950 code object -- without atomics, LDS, scratch or a fused multiply-add on the value path."""

import math
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


def test_power_smooth_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_power_smooth_n_{combo}"), combo
        assert "sdft_power_smooth_n" in capi.typed_signatures(combo)


@pytest.mark.parametrize("combo", COMBOS)
def test_power_smooth_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    for decay in (0.5, float("nan")):
        assert api.sdft_power_smooth_n(None, 100, None, 10, 0, 0, 1, decay, None, None) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_power_smooth_n" in err and "NULL plan" in err, err
        api.clear()


def test_smooth_coefficients_are_the_rounded_decay_and_its_complement():
    from sdft_amd.sdft import smooth_coefficients
    for dtype in (np.float32, np.float64):
        for decay in (0.0, 0.5, 0.9, 1.0 - 2.0 ** -10, 0.123456789, 1e-3):
            a, b = smooth_coefficients(decay, dtype)
            assert type(a) is dtype and type(b) is dtype
            assert a == dtype(decay) and b == dtype(1) - a
        assert smooth_coefficients(0.0, dtype) == (dtype(0), dtype(1))
        for bad in (float("nan"), -1e-30, -0.5, 1.0, 1.5, float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="decay"):
                smooth_coefficients(bad, dtype)
    # the float case: below 1 as a double, 1 after rounding
    near = 1.0 - 2.0 ** -26
    assert near < 1.0 and np.float32(near) == np.float32(1)
    with pytest.raises(ValueError, match="decay"):
        smooth_coefficients(near, np.float32)
    a, b = smooth_coefficients(near, np.float64)
    assert a == near and b == 2.0 ** -26


def test_smooth_decay_of_a_time_constant():
    from sdft_amd.sdft import smooth_coefficients, smooth_decay
    for tau in (0.5, 1.0, 10.0, 480.0, 48000.0, 1e9):
        d = smooth_decay(tau)
        assert d == math.exp(-1.0 / tau) and 0.0 < d < 1.0
        smooth_coefficients(d, np.float64)
    assert abs(smooth_decay(100.0) ** 100 - math.exp(-1.0)) < 1e-12       # after tau samples a step has reached 1 - 1/e
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(ValueError, match="time constant"):
            smooth_decay(bad)


def test_power_smooth_refusals_of_the_python_call_before_a_plan_is_touched(hip_library):
    """a bad grid, band or decay and a state that cannot be updated in place are refused by SDFT.power_smooth itself (the C call's
    own refusals need a plan, hence a GPU: tests/test_gpu_power_smooth.py)"""
    from sdft_amd import sdft as S

    class NoPlan:
        dftsize = 8
        channels = 1
        fd = np.float32

        class api:
            @staticmethod
            def clear():
                pass

    x = np.zeros(4, dtype=np.float32)
    for bad in (float("nan"), -0.25, 1.0, 1.0 - 2.0 ** -26, 7):
        with pytest.raises(ValueError, match="decay"):
            S.SDFT.power_smooth(NoPlan(), x, bad)
    with pytest.raises(ValueError):
        S.SDFT.power_smooth(NoPlan(), x, 0.5, every=0)
    for bins in ((0, 0), (8, 1), (1, 8)):
        with pytest.raises(ValueError):
            S.SDFT.power_smooth(NoPlan(), x, 0.5, bins=bins)
    for state in (np.zeros(8, dtype=np.float64), np.zeros(7, dtype=np.float32), np.zeros((2, 8), dtype=np.float32), np.zeros(16, dtype=np.float32)[::2],
                  [0.0] * 8):
        with pytest.raises(ValueError, match="state"):
            S.SDFT.power_smooth(NoPlan(), x, 0.5, state=state)
    frozen = np.zeros(8, dtype=np.float32)
    frozen.setflags(write=False)
    with pytest.raises(ValueError, match="state"):
        S.SDFT.power_smooth(NoPlan(), x, 0.5, state=frozen)


def test_power_smooth_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    assert "sdft_hip_sdft_power_smooth_n(" in c_header and "SDFT_HIP_SYMBOL(sdft_power_smooth_n)" in c_header
    assert "const double decay, sdft_fd_t* state, sdft_fd_t* smooth)" in c_header
    assert '("last_kernel" = 15)' in c_header and "15 (smoothed power analysis)" in c_header
    assert "8 u M / (1 - a)" in c_header
    assert "sdft_hip_sdft_power_smooth_n_##SUF" in cpp_header and "std::size_t power_smooth(" in cpp_header


def test_power_smooth_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "power_smooth_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "power_smooth_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "power-smooth-logic: all properties hold" in r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_power_smooth_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_power_smooth_kernel at the type pair's one bins-per-lane and the two kernels that
    carry the average across time chunks are in the translation unit's gfx950 code object; none of them holds an atomic, an LDS
    access or a scratch access, and the recursion, the scan and the fix-up have no fused multiply-add of the FD type.  The
    pooled-power and power kernels beside them are the sets they were."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_power_smooth_kernel")}
    assert found == {f"forward_power_smooth_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(found)
    helpers = {name for name in kernels if name.startswith(("smooth_scan_kernel", "smooth_fix_kernel"))}
    assert helpers == {f"smooth_scan_kernel<{fd}>", f"smooth_fix_kernel<{fd}>"}, sorted(helpers)
    fused = r"v_fma(c|mk|ak)?_f64|v_pk_fma" if fd == "double" else r"v_pk_fma|v_fma_f64"
    for name in found | helpers:
        ops = [line.split()[0] for line in kernels[name] if line]
        assert not [o for o in ops if "atomic" in o], name
        assert not [o for o in ops if o.startswith(("ds_", "scratch_"))], name
        assert not [o for o in ops if re.match(fused, o)], name
    pooled = {name for name in kernels if name.startswith("forward_pooled_power_kernel")}
    assert pooled == {f"forward_pooled_power_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(pooled)
    dense = {name for name in kernels if name.startswith("forward_power_kernel")}
    assert dense == {f"forward_power_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(dense)
