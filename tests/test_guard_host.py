"""CPU: the host half of the parity build's guarded device allocator (tandem_amd/csrc/guard_host.h): the poison pattern, the scan of
a guard that was copied back, the violation record and the report text.  tests/cpp/guard_check.cpp is a stand-alone program; it is
built with g++ and run under AddressSanitizer + UBSan (nothing preloaded, nothing loaded into Python).  The device half is
exercised by tests/test_guarded_gpu.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_guard_host_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "guard_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/guard_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "guard_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_guard_host_includes_no_hip_header():
    src = open(os.path.join(ROOT, "tandem_amd", "csrc", "guard_host.h")).read()
    assert not re.search(r'#include\s*[<"][^>"]*hip', src)
    assert not re.search(r'#include\s*"', src), "guard_host.h stands alone: standard headers only"


def test_the_pattern_is_a_quiet_nan_without_zero_or_ff_bytes():
    """The same facts from Python's side: the word tests/guard_helpers.py looks for is the header's, and numpy reads it as a NaN."""
    import numpy as np
    src = open(os.path.join(ROOT, "tandem_amd", "csrc", "guard_host.h")).read()
    word = int(re.search(r"kWord\s*=\s*(0x[0-9a-fA-F]+)u", src).group(1), 16)
    pat = [int(x, 16) for x in re.search(r"kPattern\[4\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")]
    assert bytes(pat) == word.to_bytes(4, "little")
    assert all(b not in (0x00, 0xff) for b in pat)
    assert np.isnan(np.array([word], np.uint32).view(np.float32)[0])
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import guard_helpers
    assert guard_helpers.POISON_WORD == word
