"""The prefix-cell route of long analysis calls without a GPU: the route's conditions in the host-side logic
(tests/cpp/prefix_logic_test.cpp under g++ -fsanitize=address,undefined) and prefix_cells_kernel in the gfx950 code objects of
the two FD double translation units."""

import os
import shutil
import subprocess

import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")


def test_prefix_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "prefix_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "prefix_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "prefix-logic: all properties hold" in r.stdout


@pytest.mark.parametrize("combo,td", (("f32f64", "float"), ("f64f64", "double")))
def test_prefix_cells_kernel_in_code_object(hip_library, combo, td):
    """FD double only: one instantiation per translation unit, by name."""
    kernels = disassemble(combo, hip_library)
    found = sorted(name for name in kernels if name.startswith("prefix_cells_kernel"))
    assert found == [f"prefix_cells_kernel<{td}, double>"], found
