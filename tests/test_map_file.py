"""CPU: the DrFusion map file (include/dr_mi355x.h "map files").  tandem_amd/csrc/map_file.h -- the streaming writer, the
validating reader -- compiled with plain g++ (tests/cpp/map_file_check.cpp) and held to a restatement of the format written
here with struct and numpy; every refusal; the same under AddressSanitizer and UBSan as a stand-alone program
(tests/cpp/map_file_san.cpp); drf_map_info, which needs no device; and tandem_amd.map_file against the same restatement."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 20
M64 = (1 << 64) - 1
u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


# ------------------------------------------------------------------ the format, restated
def pack(c):
    return ((int(c[0]) + B) << 42) | ((int(c[1]) + B) << 21) | (int(c[2]) + B)


def unpack(k):
    return ((k >> 42) & 0x1fffff) - B, ((k >> 21) & 0x1fffff) - B, (k & 0x1fffff) - B


def fnv_words(data, h=0xcbf29ce484222325):
    for w in np.frombuffer(data, "<u8").tolist():
        h = ((h ^ w) * 0x100000001b3) & M64
    return h


def compose(vs, keys, vox, **over):
    """The bytes of a map file: keys ascending ints, vox (n, 4096) uint8.  over: header fields to get wrong on purpose."""
    n = len(keys)
    body = np.asarray(keys, "<u8").tobytes() + np.ascontiguousarray(vox, np.uint8).tobytes()
    head = (over.get("magic", b"DRFMAP01") + struct.pack("<III", over.get("header", 64), over.get("edge", 8), over.get("voxel", 8))
            + np.float32(vs).tobytes() + struct.pack("<Q", over.get("n", n)) + over.get("reserved", bytes(32)))
    assert len(head) == 64
    return head + body + struct.pack("<Q", over.get("checksum", fnv_words(body)))


def parse(data):
    """(voxel_size bits, keys, vox, checksum) of a well-formed file; asserts everything the format promises."""
    assert data[:8] == b"DRFMAP01"
    hb, edge, vb, vs_bits, n = struct.unpack("<IIIIQ", data[8:32])
    assert (hb, edge, vb) == (64, 8, 8) and data[32:64] == bytes(32)
    assert len(data) == 72 + 4104 * n
    keys = np.frombuffer(data, "<u8", n, 64)
    assert n < 2 or (keys[1:] > keys[:-1]).all()
    assert n == 0 or int(keys[-1]) < (1 << 63)
    vox = np.frombuffer(data, np.uint8, 4096 * n, 64 + 8 * n).reshape(n, 4096)
    (cs,) = struct.unpack("<Q", data[-8:])
    assert cs == fnv_words(data[64:-8])
    return vs_bits, keys, vox, cs


def random_map(n, seed):
    """n blocks: the corners of the key range, negative coordinates, the rest around the origin; keys ascending."""
    rng = np.random.default_rng(seed)
    coords = set([(-(B - 1), -(B - 1), -(B - 1)), (B - 1, B - 1, B - 1), (-1, -1, -1), (-300, 7, -2), (B - 1, -(B - 1), 0)][:n])
    while len(coords) < n:
        coords.add(tuple(int(v) for v in rng.integers(-400, 400, 3)))
    keys = sorted(pack(c) for c in coords)
    vox = rng.integers(0, 256, (n, 4096), dtype=np.uint8)
    return keys, vox


VS = np.float32(0.02)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("map_file") / "libmap_file_check.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests/cpp/map_file_check.cpp"), "-o", so])
    h = C.CDLL(so)
    h.mf_last_error.restype = C.c_char_p
    h.mf_write.argtypes = [C.c_char_p, C.c_float, u64p, C.c_uint64, u8p, C.c_size_t]
    h.mf_write_abandoned.argtypes = [C.c_char_p, C.c_float, u64p, C.c_uint64]
    h.mf_info.argtypes = [C.c_char_p, C.POINTER(C.c_float), u64p]
    h.mf_read.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_float), u64p, u64p, u8p, C.c_uint64, u64p]
    h.mf_read_changed.argtypes = [C.c_char_p, C.c_int]
    return h


def cpp_write(H, path, keys, vox, chunk=0):
    k = np.ascontiguousarray(keys, np.uint64)
    v = np.ascontiguousarray(vox, np.uint8)
    return H.mf_write(str(path).encode(), VS, k.ctypes.data_as(u64p), len(k), v.ctypes.data_as(u8p), chunk)


def cpp_read(H, path, chunk, cap):
    vs, n, cs = C.c_float(), C.c_uint64(), C.c_uint64()
    keys, vox = np.zeros(max(cap, 1), np.uint64), np.zeros((max(cap, 1), 4096), np.uint8)
    rc = H.mf_read(str(path).encode(), chunk, C.byref(vs), C.byref(n), keys.ctypes.data_as(u64p), vox.ctypes.data_as(u8p), cap, C.byref(cs))
    return rc, np.float32(vs.value), keys[:n.value], vox[:n.value], cs.value


def cpp_refuses(H, path):
    vs, n = C.c_float(), C.c_uint64()
    return H.mf_info(str(path).encode(), C.byref(vs), C.byref(n)) != 0 and len(H.mf_last_error()) > 0


# ------------------------------------------------------------------ round trips
@pytest.mark.parametrize("n", [0, 1, 300])
def test_the_writer_produces_the_restated_format(H, tmp_path, n):
    keys, vox = random_map(n, seed=3 + n)
    for chunk in (0, 1, 7, 64):
        p = tmp_path / f"w{chunk}.drfmap"
        assert cpp_write(H, p, keys, vox, chunk) == 0, H.mf_last_error()
        assert not os.path.exists(str(p) + ".part")
        data = p.read_bytes()
        assert data == compose(VS, keys, vox)
        vs_bits, k, v, cs = parse(data)
        assert vs_bits == int(VS.view(np.uint32)) and list(k) == keys and np.array_equal(v, vox)
    if n:
        c = [unpack(k) for k in keys]
        assert min(min(x) for x in c) == -(B - 1) and (n < 2 or max(max(x) for x in c) == B - 1)


@pytest.mark.parametrize("n", [0, 1, 300])
def test_the_reader_reads_what_the_restatement_wrote(H, tmp_path, n):
    keys, vox = random_map(n, seed=11 + n)
    p = tmp_path / "r.drfmap"
    data = compose(VS, keys, vox)
    p.write_bytes(data)
    for chunk in (1, 7, 64, 0):
        rc, vs, k, v, cs = cpp_read(H, p, chunk, n)
        assert rc == 0, (rc, H.mf_last_error())
        assert vs.view(np.uint32) == VS.view(np.uint32) and list(k) == keys and np.array_equal(v, vox)
        assert cs == struct.unpack("<Q", data[-8:])[0]


# ------------------------------------------------------------------ refusals
def bad_files(keys, vox):
    good = compose(VS, keys, vox)
    n = len(keys)
    flip = lambda d, at, bit: d[:at] + bytes([d[at] ^ bit]) + d[at + 1:]  # noqa: E731
    reserved = bytearray(32)
    reserved[19] = 1
    body_fixed = lambda ks: compose(VS, ks, vox)  # noqa: E731  (checksum right: the key order alone refuses)
    return {
        "wrong magic": compose(VS, keys, vox, magic=b"DRFMAP02"),
        "header size": compose(VS, keys, vox, header=72),
        "block edge": compose(VS, keys, vox, edge=16),
        "voxel bytes": compose(VS, keys, vox, voxel=4),
        "reserved byte": compose(VS, keys, vox, reserved=bytes(reserved)),
        "cut in the key table": good[:64 + 8 * n - 5],
        "cut in the payload": good[:64 + 8 * n + 4096 * (n // 2) + 100],
        "cut in the trailer": good[:-3],
        "one extra byte": good + b"\0",
        "n too large": compose(VS, keys, vox, n=n + 1),
        "n absurd": compose(VS, keys, vox, n=(1 << 64) - 1),
        "two equal keys": body_fixed(keys[:5] + [keys[4]] + keys[6:]),
        "descending pair": body_fixed(keys[:5] + [keys[6], keys[5]] + keys[7:]),
        "key above 2^63": body_fixed(keys[:-1] + [(1 << 63) | keys[-1]]),
        "voxel bit": flip(good, 64 + 8 * n + 4096 * 17 + 123, 0x10),
        "checksum bit": flip(good, len(good) - 8, 0x01),
        "empty file": b"",
        "header only": good[:64],
    }


def test_every_malformed_file_is_refused(H, tmp_path):
    keys, vox = random_map(40, seed=5)
    p = tmp_path / "good.drfmap"
    p.write_bytes(compose(VS, keys, vox))
    assert not cpp_refuses(H, p)
    for what, data in bad_files(keys, vox).items():
        q = tmp_path / "bad.drfmap"
        q.write_bytes(data)
        assert cpp_refuses(H, q), what
        assert cpp_read(H, q, 7, 40)[0] == 1, what


@pytest.mark.parametrize("n", [3, 40])
def test_a_file_that_changes_between_validation_and_reading_fails_verify(H, tmp_path, n):
    """MapReader::verify: the second pass over the file -- the one whose blocks are placed -- must meet the bytes open() validated."""
    keys, vox = random_map(n, seed=21 + n)
    p = tmp_path / "v.drfmap"
    good = compose(VS, keys, vox)
    p.write_bytes(good)
    assert H.mf_read_changed(str(p).encode(), 0) == 0, H.mf_last_error()
    assert H.mf_last_error() == b""
    assert H.mf_read_changed(str(p).encode(), 1) == 5, H.mf_last_error()      # every read() succeeded, verify() did not
    assert H.mf_last_error() == f"map file {p} changed while it was read".encode()
    data = p.read_bytes()
    at = 64 + 8 * n + 4096 * (n - 1) + 2048
    assert data[at] == good[at] ^ 0x20 and data[:at] == good[:at] and data[at + 1:] == good[at + 1:]  # one byte, in the last block
    assert cpp_refuses(H, p)                                                  # and a new open() sees it


def test_a_failed_write_leaves_nothing_behind(H, tmp_path):
    keys, vox = random_map(10, seed=7)
    missing = tmp_path / "no" / "such" / "dir" / "m.drfmap"
    assert cpp_write(H, missing, keys, vox) == 1 and b"cannot create" in H.mf_last_error()
    assert not (tmp_path / "no").exists()
    p = tmp_path / "m.drfmap"
    k = np.ascontiguousarray(keys, np.uint64)
    assert H.mf_write_abandoned(str(p).encode(), VS, k.ctypes.data_as(u64p), len(k)) == 0
    assert os.listdir(tmp_path) == []                    # a writer that goes away unfinished removes its .part
    assert cpp_write(H, p, keys[::-1], vox) == 1         # the writer refuses keys out of order before it creates anything
    assert os.listdir(tmp_path) == []
    assert cpp_write(H, p, keys, vox) == 0 and os.listdir(tmp_path) == ["m.drfmap"]


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """map_file.h under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "map_file_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests/cpp/map_file_san.cpp"), "-o", exe])
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map_file_san ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


# ------------------------------------------------------------------ the C ABI and the Python module
@pytest.fixture(scope="module")
def L():
    return abi_module()


def test_abi_declares_exports_and_types_the_three_functions(L):
    src = check_symbols(L, ["drf_map_info", "drf_save_map", "drf_load_map"])
    assert "DRFMAP01" in open(os.path.join(ROOT, "include", "dr_mi355x.h")).read()
    assert "size_t chunk_blocks" in src


def test_map_info_needs_no_device(L, tmp_path):
    lib = L.lib()
    keys, vox = random_map(25, seed=9)
    p = tmp_path / "m.drfmap"
    p.write_bytes(compose(VS, keys, vox))
    vs, n = C.c_float(), C.c_uint64()
    assert lib.drf_map_info(str(p).encode(), C.byref(vs), C.byref(n)) == 0
    assert np.float32(vs.value).view(np.uint32) == VS.view(np.uint32) and n.value == 25
    for what, data in bad_files(keys, vox).items():
        q = tmp_path / "bad.drfmap"
        q.write_bytes(data)
        assert lib.drf_map_info(str(q).encode(), C.byref(vs), C.byref(n)) == 4, what
        assert b"bad.drfmap" in lib.dr_last_error(), what
    assert lib.drf_map_info(str(tmp_path / "missing.drfmap").encode(), C.byref(vs), C.byref(n)) == 4
    assert lib.drf_map_info(None, C.byref(vs), C.byref(n)) == 1
    assert lib.drf_map_info(str(p).encode(), None, C.byref(n)) == 1
    assert lib.drf_map_info(str(p).encode(), C.byref(vs), None) == 1
    assert lib.drf_save_map(None, str(p).encode(), 0) == 1 and lib.drf_load_map(None, str(p).encode(), 0) == 1


def test_python_module_against_the_restatement(L, tmp_path):
    from tandem_amd import map_file
    from tandem_amd.dr_fusion import map_info
    keys, vox = random_map(60, seed=13)
    p = tmp_path / "m.drfmap"
    p.write_bytes(compose(VS, keys, vox))
    vs, coords, v = map_file.read(p)
    assert np.float32(vs) == VS and [pack(c) for c in coords] == keys and np.array_equal(v, vox)
    assert map_info(p) == (float(VS), 60)
    # what the module writes, blocks handed over in another order, the restatement parses to the same map
    order = np.random.default_rng(1).permutation(60)
    q = tmp_path / "w.drfmap"
    map_file.write(q, VS, coords[order], vox[order])
    assert q.read_bytes() == p.read_bytes()
    parse(q.read_bytes())
    e = tmp_path / "e.drfmap"
    map_file.write(e, VS, np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.uint8))
    assert e.read_bytes() == compose(VS, [], np.zeros((0, 4096), np.uint8)) and len(e.read_bytes()) == 72
    with pytest.raises(L.DrError) as err:
        (tmp_path / "bad.drfmap").write_bytes(p.read_bytes()[:-1])
        map_file.read(tmp_path / "bad.drfmap")
    assert err.value.code == 4


def test_info_command_runs_without_a_device(L, tmp_path):
    keys, vox = random_map(30, seed=15)
    p = tmp_path / "m.drfmap"
    p.write_bytes(compose(VS, keys, vox))
    r = subprocess.run([sys.executable, "-m", "tandem_amd.map_file", "info", str(p)], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split(None, 1) for line in r.stdout.strip().splitlines())
    assert out["blocks"] == "30" and out["bytes"] == str(72 + 4104 * 30) and out["magic"] == "DRFMAP01"
    c = np.array([unpack(k) for k in keys])
    assert out["block_min"] == str([int(v) for v in c.min(0)]) and out["block_max"] == str([int(v) for v in c.max(0)])


def test_shim_program_compiles_and_links_with_gcc(L, tmp_path):
    """tests/cpp/map_io_shim.cpp (run by tests/test_fusion_map_file_gpu.py) against tandem_amd/libdr/dr_fusion.h, as C++14."""
    exe = str(tmp_path / "map_io_shim")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), os.path.join(ROOT, "tests/cpp/map_io_shim.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x",
                           "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage:" in r.stderr
