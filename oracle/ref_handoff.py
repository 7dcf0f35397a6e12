"""ctypes wrapper of oracle/_ref/libdense_handoff_ref.so -- the REFERENCE's own dense-depth hand-off (CoarseTracker::setCoarseTrackingRef,
tandem/src/FullSystem/CoarseTracker.cpp:654-723) compiled for the host by oracle/Makefile.ref.  TEST INFRASTRUCTURE: only tests/ may import this.  Without that build, dense_handoff answers
from the results recorded from it (oracle/ref_replay.py, tests/golden/ref_handoff.npz)."""
import ctypes as C
import os

import numpy as np

from oracle import ref_replay

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}
_STORE = ref_replay.Store("handoff")


def path(sum_left=False):
    return os.path.join(_HERE, "_ref", "libdense_handoff_ref_left.so" if sum_left else "libdense_handoff_ref.so")


def built():
    return os.path.isfile(path(False)) and os.path.isfile(path(True))


def available():
    """The host build, or the results recorded from it."""
    return built() or _STORE.exists()


def _lib(sum_left):
    if sum_left not in _libs:
        L = C.CDLL(path(sum_left))
        vp = C.c_void_p
        L.ref_dense_handoff.restype = C.c_int
        L.ref_dense_handoff.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        _libs[sum_left] = L
    return _libs[sum_left]


def _colour_bits(dIp0, u, v):
    """Bits of dIp0[v, u, 0] at every slot whose (u, v) is a pixel, 0 elsewhere: the block takes a point's colour from there, so the
    recorded colour is stored as its XOR with this lookup of the call's own input (mostly zeros) -- lossless whatever the block did."""
    H, W = dIp0.shape[:2]
    out = np.zeros(len(u), np.uint32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(u) & np.isfinite(v) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (u == np.floor(u)) & (v == np.floor(v))
    out[ok] = dIp0[v[ok].astype(np.int64), u[ok].astype(np.int64), 0].view(np.uint32)
    return out


def dense_handoff(depth, c2w_dense, c2w_last, K, step, dense_only, idepth0, dIp0, sparse=None, sum_left=False):
    """Runs the reference block.  sparse = (u, v, idepth, color) of the n0 points already in the list.  Returns dict(pc_n, u, v, idepth, color
    (the raw arrays, slot 0 .. pc_n INCLUSIVE: the block pre-increments), KRKi (9,), Kt (3,)): the block's own float products."""
    H, W = depth.shape
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    depth, idepth0, dIp0 = f32(depth), f32(idepth0), f32(dIp0)
    assert idepth0.shape == (H, W) and dIp0.shape == (H, W, 3)
    n0 = 0 if sparse is None else len(sparse[0])
    cap = W * H + n0 + 1
    arr = [np.full(cap, np.nan, np.float32) for _ in range(4)]
    if sparse is not None:
        for a, src in zip(arr, sparse):
            a[:n0] = src
    c2wd, c2wl, K9 = f32(c2w_dense).reshape(16), np.ascontiguousarray(c2w_last, np.float64).reshape(16), f32(K).reshape(9)
    KRKi, Kt, Ki = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(9, np.float32)
    fields = ["pc_n", "u", "v", "idepth", "color_xor_lookup", "KRKi", "Kt", "Ki"]
    key = ref_replay.digest("dense_handoff", depth, c2wd, c2wl, K9, int(step), bool(dense_only), idepth0, dIp0, [a[:n0] for a in arr], bool(sum_left))
    if not built():
        r = _STORE.get(key, fields)
        r["color"] = (r["color_xor_lookup"] ^ _colour_bits(dIp0, r["u"], r["v"])).view(np.float32)
        for a, f in zip(arr, ("u", "v", "idepth", "color")):  # recorded up to slot pc_n: the slots after it are the NaN they were filled with
            a[:len(r[f])] = r[f]
        return dict(pc_n=int(r["pc_n"]), n0=n0, u=arr[0], v=arr[1], idepth=arr[2], color=arr[3], KRKi=r["KRKi"], Kt=r["Kt"], Ki=r["Ki"])
    n = _lib(sum_left).ref_dense_handoff(W, H, depth.ctypes.data, c2wd.ctypes.data, c2wl.ctypes.data, K9.ctypes.data, step, int(dense_only), idepth0.ctypes.data,
                                          dIp0.ctypes.data, n0, *[a.ctypes.data for a in arr], KRKi.ctypes.data, Kt.ctypes.data, Ki.ctypes.data)
    res = dict(pc_n=n, n0=n0, u=arr[0], v=arr[1], idepth=arr[2], color=arr[3], KRKi=KRKi, Kt=Kt, Ki=Ki)
    if ref_replay.RECORD:
        assert all(np.isnan(a[n + 1:]).all() for a in arr), "the block wrote past slot pc_n"
        rec = {f: (res[f][:n + 1] if f in ("u", "v", "idepth") else res[f]) for f in fields if f != "color_xor_lookup"}
        rec["color_xor_lookup"] = res["color"][:n + 1].view(np.uint32) ^ _colour_bits(dIp0, rec["u"], rec["v"])
        _STORE.put(key, rec)
    return res
