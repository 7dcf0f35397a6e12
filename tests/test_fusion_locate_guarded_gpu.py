"""-m gpu: drf_locate_system and drf_locate_frame under the guarded allocator of the parity library (tests/guard_helpers.py): the
call's device scratch -- partial sums, counters, the depth image -- lies between guard bands and starts as poison, quiet NaNs.  No
guard may change, the results are bit-identical to the unguarded call and to the restatement of tests/test_map_locate.py, and no
poison word appears in them: a partial[i] that no wave wrote would reach the sums through the fold as a NaN."""
import numpy as np
import pytest

from guard_helpers import POISON_WORD, assert_same_bits, guarded
from test_fusion_map_file_gpu import engine
from test_fusion_map_locate_gpu import result_dict
from test_fusion_map_transform_gpu import write
from test_map_align import assert_same_result, assert_same_system
from test_map_locate import VS, np_locate_frame, np_locate_system, random_case

pytestmark = pytest.mark.gpu


def test_locate_under_guards(tmp_path, parity_hooks):
    """The random map of the system tests at 96x128: one evaluation at step 1 (24 groups, three of them without a sample) and at
    step 3 (a last group with tail lanes, and scratch beyond it that nobody writes or reads), and a refinement of three evaluations."""
    case = random_case(3)
    path = str(tmp_path / "m.drfmap")
    write(path, VS, *case["blocks"])
    want = [np_locate_system(case["blocks"], case["cam"], case["depth"], case["pose"], **o) for o in ({}, dict(step=3))]
    opt = dict(max_iters=3, min_valid=0.01, centre_depth=1.0)
    want_frame = np_locate_frame(case["blocks"], case["cam"], case["depth"], case["pose"], **opt)
    want_frame.pop("trace")
    assert want[0][1][1] > 0 and want_frame["iterations"] == 3

    def run():
        f = engine(case["cam"])
        f.load_map(path)
        a = f.locate_system(case["depth"], case["pose"])
        b = f.locate_system(case["depth"], case["pose"], step=3)
        r = f.locate_frame(case["depth"], case["pose"], raise_on_failure=False, **opt)
        f.close()
        assert_same_system(a, want[0], "system")
        assert_same_system(b, want[1], "system, step 3")
        assert_same_result(result_dict(r), want_frame, "refinement")
        return [("system", a[0]), ("system, step 3", b[0]), ("pose", r.T), ("pose32", r.T32), ("sums", r.sums)]

    with guarded():
        on = run()
    off = run()
    for (na, xa), (nb, xb) in zip(on, off):
        assert na == nb
        assert_same_bits(xa, xb, na)
        words = np.ascontiguousarray(xa).view(np.uint32)
        assert not (words == POISON_WORD).any(), na
