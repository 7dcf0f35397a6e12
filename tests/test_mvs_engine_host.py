"""CPU: the decisions of the DrMvsnet engine that are values with no HIP in them (tandem_amd/csrc/mvs_engine_host.h) -- WindowTicket, the
count of windows in flight; ResultSlots, the reference's call protocol without its threads; ForwardCursor, what forward() does for
each op of the plan (fork, feature cache, view-shard collectives, ranges); the page-locked span predicate -- checked by the
stand-alone program tests/cpp/mvs_engine_host_check.cpp: plain g++ -Wall -Werror, and once more under AddressSanitizer and UBSan.
A plain executable with its own main: nothing preloaded, nothing loaded into Python.  The cases are listed in the program;
DESIGN.md "Where the engine's parts live"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mvs_engine_host_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan+ubsan"])
def test_ticket_slots_cursor_and_span(tmp_path, flags):
    exe = str(tmp_path / "mvs_engine_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + flags + [SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mvs_engine_host_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
