"""CPU: the selection network of the edge measure (tandem_amd/csrc/edge_network.h, the list edge_pixel expands) checked by the zero-one principle.
tests/cpp/edge_network_check.cpp expands the same X-macro over 64-bit lanes (min = AND, max = OR) for all 2^25 zero-one inputs: wire 14 must be 1 exactly
when at least 11 inputs are 1 -- the 15th smallest of 25, ties included.  The program also runs three mutated networks and must find each wrong; asked
for one of them alone it exits with status 1, so the checker itself can be seen to fail.  g++ -Wall -Werror, no HIP header, no device; the same source
runs as a stand-alone program under ASan + UBSan."""
import os
import re
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "edge_network_check.cpp")
HEADER = os.path.join(ROOT, "tandem_amd", "csrc", "edge_network.h")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("edge_network_check") / "edge_network_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", path])
    return path


def test_wire_14_is_the_15th_smallest_for_all_zero_one_inputs(exe):
    t0 = time.perf_counter()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    took = time.perf_counter() - t0
    assert r.returncode == 0 and "edge_network_check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "113 comparators" in r.stdout
    assert "macro: 0 of 33554432 inputs wrong" in r.stdout and "table: 0 of 33554432 inputs wrong" in r.stdout, r.stdout
    print("\n%s(%.2f s)" % (r.stdout, took))


@pytest.mark.parametrize("mutant", ["drop-last", "swap-pair", "reversed"])
def test_a_mutated_network_fails_the_check(exe, mutant):
    r = subprocess.run([exe, mutant], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    wrong = int(re.match(r"%s: (\d+) of 33554432 inputs wrong" % mutant, r.stdout).group(1))
    assert wrong > 0


def test_the_header_has_no_hip_in_it_and_the_kernel_expands_it():
    text = open(HEADER).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "#include" not in code and "__device__" not in code and "hip" not in code.lower()
    kern = open(os.path.join(ROOT, "tandem_amd", "csrc", "mvs_kernels.h")).read()
    assert "DR_EDGE_NETWORK(CE)" in kern and '#include "edge_network.h"' in kern
    assert not re.search(r"CE\(\d+,\s*\d+\)", kern), "a comparator list outside edge_network.h"


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """The checker under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    path = str(tmp_path / "edge_network_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           SRC, "-o", path])
    r = subprocess.run([path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "edge_network_check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
