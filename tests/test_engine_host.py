"""CPU: two decisions of the DrFusion engine that are values with no HIP in them (tandem_amd/csrc/engine_host.h) -- CallOrder, the
order in which the engine's calls may come, and LocateStageCursor, when a map-scope localisation selects and stages stored blocks
again -- checked by the stand-alone program tests/cpp/engine_host_check.cpp: plain g++ -Wall -Werror, and once more under
AddressSanitizer and UBSan.  A plain executable with its own main: nothing preloaded, nothing loaded into Python.  The cases are
listed in the program; DESIGN.md "Where rendering and the frame pose live"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "engine_host_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan+ubsan"])
def test_call_order_and_locate_stage_cursor(tmp_path, flags):
    exe = str(tmp_path / "engine_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "engine_host_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
