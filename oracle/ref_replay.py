"""Recorded results of the reference's host build (oracle/_ref), for checkouts that cannot build it.  TEST INFRASTRUCTURE.

oracle/ref_tracker.py and oracle/ref_handoff.py call the reference's own kernels compiled for the host.  Where that build exists,
every call runs it, and with DR_REF_RECORD=1 its result is also stored in tests/golden/ref_<name>.npz, keyed by a digest of the
call's inputs.  Where it does not exist (the reference sources were not there at build time), the same call is answered from that
file: the tests synthesise their inputs deterministically (synth/), so a recorded call is found again; a call that was never recorded
is an error, never a skip.  The tests assert exactly what they assert against the live build."""
import hashlib
import lzma
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
RECORD = os.environ.get("DR_REF_RECORD") == "1"


def digest(*args):
    """sha1 over the call's arguments: arrays by dtype, shape and bytes, numbers by their exact value."""
    h = hashlib.sha1()

    def feed(a):
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            h.update(("%s%s:" % (a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        elif isinstance(a, (list, tuple)):
            h.update(b"(")
            for x in a:
                feed(x)
            h.update(b")")
        elif a is None or isinstance(a, (bool, np.bool_, str)):
            h.update(repr(a if not isinstance(a, np.bool_) else bool(a)).encode())
        elif isinstance(a, (int, np.integer)):
            h.update(b"i%d" % int(a))
        else:
            h.update(("f" + float(a).hex()).encode())
        h.update(b"|")
    for a in args:
        feed(a)
    return h.hexdigest()[:24]


def pack(a):
    """Lossless: 4- and 8-byte elements as differences of their bit patterns (modulo 2^32 / 2^64; neighbouring floats of a smooth
    field differ in their low bits only), split into byte planes, lzma.  -> uint8 array that carries dtype and shape."""
    a = np.asarray(a, order="C")
    head = ("%s;%s;" % (a.dtype.str, ",".join(str(x) for x in a.shape))).encode()
    flat, k = a.reshape(-1), a.dtype.itemsize
    if k in (4, 8) and flat.size > 1:
        u = flat.view("<u%d" % k)
        body = np.diff(u, prepend=u.dtype.type(0)).view(np.uint8).reshape(-1, k).T.tobytes()
    else:
        body = flat.tobytes()
    return np.frombuffer(head + lzma.compress(body, preset=9), np.uint8)


def unpack(b):
    dt, shape, body = np.asarray(b).tobytes().split(b";", 2)
    dt, shape = np.dtype(dt.decode()), tuple(int(x) for x in shape.decode().split(",") if x)
    body, n, k = lzma.decompress(body), int(np.prod(shape)), np.dtype(dt).itemsize
    if k in (4, 8) and n > 1:
        d = np.frombuffer(body, np.uint8).reshape(k, n).T.copy().view("<u%d" % k).reshape(n)
        flat = np.cumsum(d, dtype=d.dtype).view(dt)
    else:
        flat = np.frombuffer(body, dt)
    return flat.reshape(shape).copy()


class Store:
    """tests/golden/ref_<name>.npz: entry <digest>__<field> per recorded array, holding the name of its content entry a_<sha1>, which
    holds the array packed (pack()); arrays that several calls share are stored once.  An array close to one stored before (the two
    summation orders of one hand-off differ in a few ulp) is stored as the XOR of their bits, with b_<sha1> naming the other one."""

    def __init__(self, name):
        self.path = os.path.join(GOLDEN, "ref_%s.npz" % name)
        self._d = None

    def _load(self):
        if self._d is None:
            self._d = {}
            if os.path.isfile(self.path):
                with np.load(self.path) as z:
                    self._d = {k: z[k] for k in z.files}
        return self._d

    def exists(self):
        return os.path.isfile(self.path)

    def get(self, key, fields):
        d = self._load()
        missing = [f for f in fields if key + "__" + f not in d]
        if missing:
            raise KeyError("no recorded reference result for call %s in %s (record it with DR_REF_RECORD=1 where oracle/_ref is built)"
                           % (key, os.path.relpath(self.path, os.path.dirname(GOLDEN))))
        return {f: self._array(str(d[key + "__" + f])) for f in fields}

    def _array(self, name):
        d = self._load()
        a = unpack(d[name])
        if "b" + name[1:] in d:
            b = self._array(str(d["b" + name[1:]]))
            u = "<u%d" % b.dtype.itemsize
            a = (a ^ b.view(u)).view(b.dtype)
        return a

    def put(self, key, fields):
        d = self._load()
        for f, v in fields.items():
            v = np.asarray(v, order="C")
            name = "a_" + digest(v)
            if name not in d:
                best, base = pack(v), None
                if v.dtype.itemsize in (4, 8) and v.size > 1024:
                    u = "<u%d" % v.dtype.itemsize
                    for other in [k for k in d if k.startswith("a_")]:
                        b = self._array(other)
                        if b.dtype == v.dtype and b.shape == v.shape:
                            px = pack(v.view(u) ^ b.view(u))
                            if len(px) < len(best):
                                best, base = px, other
                d[name] = best
                if base is not None:
                    d["b" + name[1:]] = np.array(base)
                back = self._array(name)
                assert back.dtype == v.dtype and back.shape == v.shape and back.tobytes() == v.tobytes()
            d[key + "__" + f] = np.array(name)
        np.savez(self.path, **d)
