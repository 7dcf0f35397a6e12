"""-m gpu: the SCATTER (plane-major) order of k_conv_m's Winograd consumer (tandem_amd/csrc/conv_march.h march_consumer_ws) beside the
gather order it replaces (march_consumer_w), both in the parity library: DR_MARCH_W_ORDER=2 / 1 selects the order of one and the same plan.

Every case forces the Winograd marching plan the way tests/test_conv_gpu.py forces a plan candidate (DR_CONV_WINO=2, DR_CONV_RANK=0) and
runs under the guard-banded, poisoned buffers of guard_helpers.py.  Required: the two orders give the same bits (per accumulator the
MFMAs arrive in the same order), both agree with torch conv3d inside the 2e-5 bound of the direct kernels, no guard is touched, no
output element keeps the poison, and no ring wait gives up (drm_debug_conv fails when k_conv_m raised *err).

The layers are far smaller than a tile (DR_MARCH_ANY_TILE lifts the planner's "no tile more than twice the layer" rule in the parity
library; DR_CONV_NO_TAP_PRUNE keeps the three z taps of a one-plane volume): what they exercise is the walk, not the size.  The host
emulation (tests/test_march_scatter.py) runs the same shapes and reports how their step ranges fall on the columns."""
import numpy as np
import pytest

import test_conv_gpu as TC
from guard_helpers import assert_no_nan, bits, guarded

pytestmark = pytest.mark.gpu

# (Cin, Cout, D, H, W), residual add, what it exercises
CASES = [
    ((16, 8, 1, 4, 16), False, "D = 1: only dz = 1 exists"),
    ((16, 8, 2, 4, 16), False, "D = 2"),
    ((16, 8, 3, 6, 40), False, "partial x tile, three live sets exactly once"),
    ((8, 8, 8, 8, 32), False, "the stage-3 instance; every workgroup starts inside the column"),
    ((32, 8, 5, 8, 32), False, "two channel passes through raw partial sums"),
    ((16, 16, 4, 8, 32), False, "the conv2 instance, no XPAIR"),
    ((16, 8, 6, 16, 64), False, "12 steps on 16 workgroups: ranges begin in the middle of a column (za > 0)"),
    ((16, 8, 3, 96, 480), False, "270 steps on 256 workgroups: ranges that span two columns"),
    ((16, 16, 4, 8, 32), True, "residual add (add_mode 1)"),
]


@pytest.mark.parametrize("shape,with_add,what", CASES, ids=["%dto%d_%dx%dx%d%s" % (c[0] + ("_add" if c[1] else "",)) for c in CASES])
def test_scatter_order_matches_gather_order_and_torch(shape, with_add, what, monkeypatch, capfd, parity_hooks):
    from tandem_amd.dr_mvsnet import debug_conv
    cin, cout, D, H, W = shape
    rng = np.random.RandomState(1000 * cin + 100 * cout + 10 * D + H + W + int(with_add))
    x = rng.randn(D, H, W, cin).astype(np.float32)
    w = (rng.randn(cout, cin, 3, 3, 3) / np.sqrt(cin * 27)).astype(np.float32)
    scale = (1.0 + 0.3 * rng.randn(cout)).astype(np.float32)
    bias = (0.2 * rng.randn(cout)).astype(np.float32)
    add = rng.randn(D, H, W, cout).astype(np.float32) if with_add else None
    ref = TC.torch_ref(x, w, (1, 1, 1), False, scale, bias, True, add, "same" if with_add else "none")
    for k, v in dict(DR_CONV_WINO="2", DR_CONV_RANK="0", DR_CONV_PRINT="1", DR_MARCH_ANY_TILE="1", DR_CONV_NO_TAP_PRUNE="1").items():
        monkeypatch.setenv(k, v)
    got = {}
    for order, name in ((2, "scatter order"), (1, "gather order")):
        monkeypatch.setenv("DR_MARCH_W_ORDER", str(order))
        with guarded():
            y = debug_conv(x, w, (1, 1, 1), False, scale, bias, True, add, False)
        line = [l for l in capfd.readouterr().err.splitlines() if l.startswith("debug_conv:")]
        assert len(line) == 1 and line[0].split()[1].startswith("winomarch<") and line[0].endswith(", " + name), (what, line)
        assert_no_nan(y, "%s, %s" % (what, name))
        err = np.abs(y - ref).max()
        print("%s, %s: max|err| %.3e (bound %.3e)" % (what, name, err, 2e-5 * max(1.0, np.abs(ref).max())))
        assert y.shape == ref.shape and err <= 2e-5 * max(1.0, np.abs(ref).max()), "%s, %s: max|err| %.3e" % (what, name, err)
        got[order] = y
    differ = int((bits(got[2]) != bits(got[1])).sum())
    assert differ == 0, "%s: %d of %d elements differ between the scatter and the gather order" % (what, differ, got[1].size)
