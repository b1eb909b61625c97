"""Smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n) without a GPU: the symbol of every type pair, the NULL-plan error, the
refusals SDFT.smooth_peak makes before it touches a plan, the declarations in the headers, the host-side logic (kernel id, route
and time chunks, the refusals' order, the carry pass's grid, the carries-first scheme against the sequential loop and the exact
recursion; tests/cpp/smooth_peak_logic_test.cpp under g++ -fsanitize=address,undefined) and the kernel's instantiations in every
translation unit's gfx950 code object -- without atomics, LDS, scratch or a fused multiply-add on the value path."""

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


def test_smooth_peak_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_smooth_peak_n_{combo}"), combo
        assert "sdft_smooth_peak_n" in capi.typed_signatures(combo)


@pytest.mark.parametrize("combo", COMBOS)
def test_smooth_peak_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    for decay, hold in ((0.5, 0), (float("nan"), 1), (0.5, 7)):
        assert api.sdft_smooth_peak_n(None, 100, None, 10, 0, 0, 1, decay, hold, None, None) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_smooth_peak_n" in err and "NULL plan" in err, err
        api.clear()


def test_smooth_peak_refusals_of_the_python_call_before_a_plan_is_touched(hip_library):
    """a bad grid, band, hold or decay and a state that cannot be updated in place are refused by SDFT.smooth_peak itself (the C
    call's own refusals need a plan, hence a GPU: tests/test_gpu_smooth_peak.py)"""
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
            S.SDFT.smooth_peak(NoPlan(), x, bad)
    for bad in (2, -1, "peak", None):
        with pytest.raises(ValueError, match="hold"):
            S.SDFT.smooth_peak(NoPlan(), x, 0.5, hold=bad)
    with pytest.raises(ValueError):
        S.SDFT.smooth_peak(NoPlan(), x, 0.5, every=0)
    for bins in ((0, 0), (8, 1), (1, 8)):
        with pytest.raises(ValueError):
            S.SDFT.smooth_peak(NoPlan(), x, 0.5, bins=bins)
    for state in (np.zeros(8, dtype=np.float64), np.zeros(7, dtype=np.float32), np.zeros((2, 8), dtype=np.float32), np.zeros(16, dtype=np.float32)[::2],
                  [0.0] * 8):
        with pytest.raises(ValueError, match="state"):
            S.SDFT.smooth_peak(NoPlan(), x, 0.5, hold="min", state=state)
    frozen = np.zeros(8, dtype=np.float32)
    frozen.setflags(write=False)
    with pytest.raises(ValueError, match="state"):
        S.SDFT.smooth_peak(NoPlan(), x, 0.5, state=frozen)


def test_smooth_peak_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    assert "sdft_hip_sdft_smooth_peak_n(" in c_header and "SDFT_HIP_SYMBOL(sdft_smooth_peak_n)" in c_header
    assert re.search(r"const double decay, const int hold,\s+sdft_fd_t\* state, sdft_fd_t\* peaks\)", c_header)
    assert '("last_kernel" = 17)' in c_header and "17 (smoothed peak-hold analysis)" in c_header
    assert "|peaks - peak| <= 8 u M / (1 - a)" in c_header
    assert "sdft_hip_sdft_smooth_peak_n_##SUF" in cpp_header and "std::size_t smooth_peak(" in cpp_header


def test_smooth_peak_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "smooth_peak_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "smooth_peak_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "smooth-peak-logic: all properties hold" in r.stdout
    # the ratio the README quotes is the one the program prints
    worst = re.search(r"worst ratio to u M / \(1 - a\): (\d+\.\d+)", r.stdout).group(1)
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"largest ratio to u·M/(1−a) of **{worst}**" in fh.read(), worst


@pytest.mark.parametrize("combo", COMBOS)
def test_smooth_peak_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_smooth_peak_kernel for either hold, at the type pair's one bins-per-lane, are in
    the translation unit's gfx950 code object; none of them holds an atomic, an LDS access or a scratch access, and the recursion
    has no fused multiply-add of the FD type.  The peak-hold and smoothed power kernels beside them, and the kernels that carry the
    average across chunks and join cut windows, are the sets they were."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_smooth_peak_kernel")}
    assert found == {f"forward_smooth_peak_kernel<{fd}, {bpl}, {w}, {h}>" for w in range(4) for h in range(2)}, sorted(found)
    fused = r"v_fma(c|mk|ak)?_f64|v_pk_fma" if fd == "double" else r"v_pk_fma|v_fma_f64"
    for name in found:
        ops = [line.split()[0] for line in kernels[name] if line]
        assert not [o for o in ops if "atomic" in o], name
        assert not [o for o in ops if o.startswith(("ds_", "scratch_"))], name
        assert not [o for o in ops if re.match(fused, o)], name
    peak = {name for name in kernels if name.startswith("forward_power_peak_kernel")}
    assert peak == {f"forward_power_peak_kernel<{fd}, {bpl}, {w}, {h}>" for w in range(4) for h in range(2)}, sorted(peak)
    smooth = {name for name in kernels if name.startswith("forward_power_smooth_kernel")}
    assert smooth == {f"forward_power_smooth_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(smooth)
    helpers = {name for name in kernels if name.startswith(("smooth_scan_kernel", "smooth_fix_kernel", "peak_rows_kernel"))}
    assert helpers == {f"{k}<{fd}>" for k in ("smooth_scan_kernel", "smooth_fix_kernel", "peak_rows_kernel")}, sorted(helpers)
    assert [name for name in kernels if name.startswith(f"peak_join_kernel<{fd}>")]
