"""CPU: the streaming surface of the C ABI (drf_streaming_min_radius, drf_set_streaming, drf_stream_{out,in}_region,
drf_streaming_stats, drf_export_host_blocks) is declared, exported and typed; the minimum radius is the bound DESIGN.md
derives; null and invalid arguments are refused without a device."""
import ctypes as C
import math
import os

import pytest

from fusion_helpers import abi_module, check_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("drf_streaming_min_radius", "drf_set_streaming", "drf_stream_out_region", "drf_stream_in_region", "drf_streaming_stats",
       "drf_export_host_blocks")


@pytest.fixture(scope="module")
def L():
    return abi_module()


def restated_min_radius(o):
    """DESIGN.md "Streaming voxel blocks": max(D rho + trunc + 4.5 s, 12.5 s) + 8 s + vs, s = sqrt(3) vs."""
    rho = max(math.sqrt(((u - o["cx"]) / o["fx"]) ** 2 + ((v - o["cy"]) / o["fy"]) ** 2 + 1.0)
              for u in (0, o["width"] - 1) for v in (0, o["height"] - 1))
    s = math.sqrt(3.0) * o["voxel_size"]
    return max(o["max_sensor_depth"] * rho + o["truncation_distance"] + 4.5 * s, 12.5 * s) + 8 * s + o["voxel_size"]


def opts(**kw):
    d = dict(voxel_size=0.01, num_buckets=1000, bucket_size=10, num_blocks=1000, block_size=8, max_sdf_weight=64,
             truncation_distance=0.04, max_sensor_depth=10.0, min_sensor_depth=0.1, num_render_streams=1,
             fx=500.0, fy=500.0, cx=319.5, cy=239.5, height=480, width=640)
    d.update(kw)
    return d


def f32(x):
    return C.c_float(x).value


def test_symbols_declared_exported_and_typed(L):
    check_symbols(L, NEW)


@pytest.mark.parametrize("kw", [
    dict(),                                                                  # TANDEM: 640x480, 1 cm, 10 m -> about 13 m
    dict(max_sensor_depth=2.5),
    dict(voxel_size=0.02, truncation_distance=0.08, max_sensor_depth=2.0, fx=100.0, fy=100.0, cx=63.5, cy=47.5, height=96, width=128),
    dict(voxel_size=0.005, truncation_distance=0.02, max_sensor_depth=4.0, fx=320.0, fy=330.0, cx=100.0, cy=300.0),  # off-centre principal point
    dict(voxel_size=0.05, truncation_distance=0.0, max_sensor_depth=0.2),    # the shifted start block dominates
])
def test_min_radius_equals_the_derived_bound(L, kw):
    o = opts(**kw)
    r = C.c_float()
    assert L.lib().drf_streaming_min_radius(C.byref(L.FusionOptions(**o)), C.byref(r)) == 0
    want = restated_min_radius({k: f32(v) if isinstance(v, float) else v for k, v in o.items()})
    assert r.value == pytest.approx(want, rel=1e-6, abs=0)
    if not kw:
        assert 12.9 < r.value < 13.2


def test_min_radius_rejects_null_and_invalid_options(L):
    lib = L.lib()
    r = C.c_float()
    assert lib.drf_streaming_min_radius(None, C.byref(r)) == 1
    assert lib.drf_streaming_min_radius(C.byref(L.FusionOptions(**opts())), None) == 1
    for bad in (dict(voxel_size=0.0), dict(fx=-1.0), dict(fy=0.0), dict(width=0), dict(height=-4), dict(max_sensor_depth=0.0),
                dict(max_sensor_depth=float("nan")), dict(truncation_distance=-0.1), dict(cx=float("inf"))):
        assert lib.drf_streaming_min_radius(C.byref(L.FusionOptions(**opts(**bad))), C.byref(r)) == 1, bad


def test_streaming_calls_reject_a_null_handle(L):
    lib = L.lib()
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    out = (C.c_uint64 * 6)()
    n = C.c_int()
    assert lib.drf_set_streaming(None, 5.0, 0) == 1
    assert lib.drf_stream_out_region(None, lo, hi) == 1
    assert lib.drf_stream_in_region(None, lo, hi) == 1
    assert lib.drf_streaming_stats(None, out) == 1
    assert lib.drf_export_host_blocks(None, 0, None, None, C.byref(n)) == 1
    assert "NULL handle" in lib.dr_last_error().decode()
