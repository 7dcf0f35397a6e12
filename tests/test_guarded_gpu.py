"""-m gpu: the FOOTPRINT of the kernels.  Every other GPU test asks whether the values a kernel wrote where it was supposed to write are
right; these ask whether it wrote anywhere else, and whether it read something nobody had written.  The parity library's allocator
(tandem_amd/csrc/dr_common.h, guard_host.h) puts a guard band on either side of every device allocation and fills guards and payload with a
pattern whose aligned words are quiet NaNs.  A store outside a tensor changes a guard (named at exit of `guarded()`: buffer, side, byte
offset); a read of a never-written element is a NaN that propagates into the output.

Every test runs its calls once under guards and once, in the same library, with guards off, and requires the outputs to be equal bit
for bit and free of NaN: poison and guards may change nothing.  The values themselves are held to the references the existing tests use
(torch for the convolutions, the CPU oracles for DrFusion and the tracker).  Shapes are the smallest with partial tiles in every axis."""
import ctypes as C

import numpy as np
import pytest

import mvs_stage_ref as R
from guard_helpers import assert_no_nan, assert_same_bits, check, guarded

pytestmark = pytest.mark.gpu


def on_and_off(run, what):
    """run() -> list of (name, array): once under guards, once without; bit-identical.  Returns the guarded outputs."""
    with guarded():
        a = run()
    b = run()
    assert len(a) == len(b) and len(a) > 0, (what, len(a), len(b))
    for (na, xa), (nb, xb) in zip(a, b):
        assert na == nb, (what, na, nb)
        assert_same_bits(xa, xb, "%s: %s" % (what, na))
    return a


# ------------------------------------------------------------------ a. the detector fires
def test_the_detector_fires(parity_hooks):
    """One byte behind a 1000-byte buffer and one byte before it, written with dr_memcpy_h2d (both inside the allocation: nothing faults)."""
    from tandem_amd import _lib
    L = _lib.lib()
    _lib.check(L.dr_guard_clear())
    assert L.dr_guard_set(1000) == 1                      # DR_ERR_ARG: no multiple of 4096
    _lib.check(L.dr_guard_set(4096))
    d = C.c_void_p()
    try:
        _lib.check(L.dr_device_alloc(0, 1000, C.byref(d)))
    finally:
        _lib.check(L.dr_guard_set(0))
    st, rep = check()
    assert st == dict(live=1, guarded=1, violations=0, bytes=1000) and rep == "", (st, rep)
    # the payload starts as the pattern: every aligned word the quiet NaN
    back = np.zeros(250, np.uint32)
    _lib.check(L.dr_memcpy_d2h(back.ctypes.data_as(C.c_void_p), d, 1000))
    assert (back == 0x7FC5A5A5).all() and np.isnan(back.view(np.float32)).all()
    one = np.zeros(1, np.uint8)
    _lib.check(L.dr_memcpy_h2d(C.c_void_p(d.value + 1000), one.ctypes.data_as(C.c_void_p), 1))
    _lib.check(L.dr_memcpy_h2d(C.c_void_p(d.value - 1), one.ctypes.data_as(C.c_void_p), 1))
    st, rep = check()
    print(rep)
    assert st["violations"] == 2 and st["live"] == 1, (st, rep)
    lines = sorted(rep.splitlines())
    assert lines == ["dr_device_alloc (1000 bytes): back guard, 1 byte changed, offsets +0..+0",
                     "dr_device_alloc (1000 bytes): front guard, 1 byte changed, offsets -1..-1"], rep
    # the check at free finds the same two, and they stay until cleared
    _lib.check(L.dr_device_free(d))
    st, rep2 = check()
    assert st["violations"] == 2 and st["live"] == 0 and st["bytes"] == 0 and sorted(rep2.splitlines()) == lines, (st, rep2)
    _lib.check(L.dr_guard_clear())
    st, rep = check()
    assert st == dict(live=0, guarded=0, violations=0, bytes=0) and rep == "", (st, rep)
    # a truncated report is still terminated
    small = C.create_string_buffer(b"x" * 8, 8)
    out = (C.c_uint64 * 4)()
    _lib.check(L.dr_guard_check(out, small, 8))
    assert small.value == b""


def test_without_guards_and_in_the_product_library(parity_hooks):
    from tandem_amd import _lib
    L = _lib.lib()
    # guards off in the parity library: an allocation is the plain one and nothing is counted
    _lib.check(L.dr_guard_clear())
    _lib.check(L.dr_guard_set(0))
    d = C.c_void_p()
    _lib.check(L.dr_device_alloc(0, 1000, C.byref(d)))
    st, rep = check()
    assert st == dict(live=0, guarded=0, violations=0, bytes=0) and rep == "", (st, rep)
    _lib.check(L.dr_device_free(d))
    # a block that allocates nothing under guards does not pass
    with pytest.raises(AssertionError, match="nothing was allocated under guards"):
        with guarded():
            pass
    # the product library: all three are DR_ERR_UNSUPPORTED, and its allocations are untouched
    _lib.switch(None)
    try:
        P = _lib.lib()
        out = (C.c_uint64 * 4)()
        assert P.dr_guard_set(4096) == 6 and P.dr_guard_clear() == 6 and P.dr_guard_check(out, None, 0) == 6
        assert b"parity library" in P.dr_last_error()
        _lib.check(P.dr_device_alloc(0, 1000, C.byref(d)))
        _lib.check(P.dr_device_free(d))
    finally:
        _lib.switch(_lib.HOOKS_LIB_PATH)


# ------------------------------------------------------------------ b. the convolution families
import test_conv_gpu as TC  # noqa: E402


def _case(table, name, dims=None, rename=None):
    c = [c for c in table if c[0].startswith(name)]
    assert len(c) == 1, (name, [x[0] for x in c])
    c = list(c[0])
    if dims:
        c[1] = dims
    if rename:
        c[0] = rename
    return tuple(c)


CONV5 = ("guard 5x5s2 8->16 ragged", (2, 18, 44), 8, 16, (1, 5, 5), (1, 2, 2), False, True, "none")
SWEEP_CUT = _case(TC.SWEEP, "sweep 3x3x3 s2 8->16", (5, 9, 22), "guard 3x3x3 s2 8->16 cut")
SKIP3 = _case(TC.CASES, "fn.skip3 1x1 8->32 +up2")
FAMILIES = {
    # id: (cases, environment, ranks, kind that must lead, kind that must have run at least once, bound)
    "k_conv": ([_case(TC.CASES, "cr.conv5 32->64 s2 odd"), SKIP3, _case(TC.CASES, "cr.prob 8->1 x8 D=4"), CONV5],
               dict(DR_CONV_ASYNC="0", DR_CONV_MARCH="0", DR_CONV_ROWMARCH="0", DR_CONV_WINO="0"), [0], "sync", "sync", 2e-5),
    "k_conv_a": ([CONV5, SWEEP_CUT, SKIP3], dict(DR_CONV_ASYNC="1", DR_CONV_MARCH="0", DR_CONV_ROWMARCH="0", DR_CONV_WINO="0"),
                 list(range(0, 40, 4)), None, "async", 2e-5),
    "k_conv_m": ([_case(TC.MARCH, "march odd sizes")], dict(DR_CONV_MARCH="2"), list(range(8)), "march", "march", 2e-5),
    "rowmarch": ([_case(TC.ROWMARCH, "rows ragged"), _case(TC.ROWMARCH, "rows one-row image")], dict(DR_CONV_ROWMARCH="2"), list(range(10)),
                 "rowmarch", "rowmarch", 2e-5),
    "k_conv_w": ([_case(TC.WINO, "wino ragged"), _case(TC.WINO, "wino two-row image")], dict(DR_CONV_WINO="2"), list(range(0, 36, 2)),
                 "wino", "wino", 2e-5),
    "winomarch": ([_case(TC.WINO_MARCH, "winomarch ragged")], dict(DR_CONV_WINO="2"), list(range(6)), "winomarch", "winomarch", 2e-5),
    "deconv form 0": ([_case(TC.CLASS_LOOP, "class loop 16->8 ragged")], dict(DR_DECONV_FORM="0"), list(range(0, 60, 6)), None, None, 2e-5),
    "deconv form 1": ([_case(TC.CLASS_LOOP, "class loop 16->8 ragged")], dict(DR_DECONV_FORM="1"), list(range(0, 60, 6)), None, None, 2e-5),
    "deconv form 2": ([_case(TC.CLASS_LOOP, "class loop 16->8 ragged")], dict(DR_DECONV_FORM="2"), list(range(0, 60, 6)), None, None, 2e-5),
    # (its own bound: the three-term bf16 split, tests/test_conv_gpu.py::test_bf16x3_conv_matches_torch)
    "bf16x3": ([SWEEP_CUT], dict(DR_CONV_BF16X3="1"), [0, 3, 6], "bf16x3", "bf16x3", 1e-4),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_convolution_families(family, monkeypatch, capfd, parity_hooks):
    """drm_debug_conv against torch_ref (test_conv_gpu.run_case and its bound) with the output starting as poison: a position no launch
    writes fails against torch, a store outside the output changes a guard of it or of a neighbour (input, weights, tap tables)."""
    import tandem_amd.dr_mvsnet as M
    cases, env, ranks, lead, must, tol = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DR_CONV_PRINT", "1")
    real, got = M.debug_conv, []

    def recording(*a, **kw):
        y = real(*a, **kw)
        got.append(y)
        return y
    monkeypatch.setattr(M, "debug_conv", recording)
    kinds_by_case = {}

    def run():
        del got[:]
        names = []
        for case in cases:
            if tol != 2e-5:
                TC._REF_CACHE.pop(case[0], None)  # (the bf16 x 3 cases keep no fp32 reference around, as in test_conv_gpu.py)
            for rank in ranks:
                monkeypatch.setenv("DR_CONV_RANK", str(rank))
                TC.run_case(case, rel_tol=tol)
                err = capfd.readouterr().err
                kinds_by_case.setdefault(case[0], []).extend(l.split()[1].split("<")[0] for l in err.splitlines() if l.startswith("debug_conv:"))
                names.append("%s rank %d" % (case[0], rank))
        assert len(got) == len(names)
        return list(zip(names, list(got)))
    on_and_off(run, family)
    for name, kinds in kinds_by_case.items():
        print(family, name, kinds)
        assert len(kinds) == 2 * len(ranks)
        if lead:
            assert kinds[0] == lead, (name, kinds)
        if must:
            assert must in kinds, "%s: %s never ran (%s)" % (name, must, kinds)


def test_class_loop_under_guards(monkeypatch, capfd, parity_hooks):
    """k_conv's class loop against the class-per-workgroup launch of the same plan, as test_class_loop_is_bit_identical: same bits."""
    from tandem_amd.dr_mvsnet import debug_conv
    name, dims, cin, cout, k, stride, transposed, relu, add_mode = _case(TC.CLASS_LOOP, "class loop 16->8 ragged")
    rng = np.random.RandomState(7)
    x = rng.randn(*dims, cin).astype(np.float32)
    w = (rng.randn(cin, cout, *k) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    scale = (1.0 + 0.3 * rng.randn(cout)).astype(np.float32)
    bias = (0.2 * rng.randn(cout)).astype(np.float32)
    add = rng.randn(*(d * 2 for d in dims), cout).astype(np.float32)
    ref = TC.torch_ref(x, w, stride, transposed, scale, bias, relu, add, add_mode)
    monkeypatch.setenv("DR_CONV_PRINT", "1")
    looped = []

    def run():
        outs = []
        for rank in range(0, 40, 4):
            monkeypatch.setenv("DR_CONV_RANK", str(rank))
            monkeypatch.delenv("DR_CONV_NO_CLASS_LOOP", raising=False)
            a = debug_conv(x, w, stride, transposed, scale, bias, relu, add, False)
            looped.append("class loop" in capfd.readouterr().err)
            monkeypatch.setenv("DR_CONV_NO_CLASS_LOOP", "1")
            b = debug_conv(x, w, stride, transposed, scale, bias, relu, add, False)
            assert "class loop" not in capfd.readouterr().err
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "candidate %d: class loop differs from class per workgroup" % rank
            assert np.abs(a - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
            outs.append(("rank %d" % rank, a))
        return outs
    on_and_off(run, "class loop")
    assert any(looped), "no candidate took the class loop"


@pytest.mark.parametrize("case", [c for c in TC.UP2 if c[0] in ("up2 16->16 ragged", "up2 one row")], ids=["ragged", "one row"])
def test_conv_over_upsampled_input_under_guards(case, monkeypatch, parity_hooks):
    import torch
    import torch.nn.functional as F
    from tandem_amd.dr_mvsnet import debug_conv
    name, dims, cin, cout = case
    rng = np.random.RandomState(len(name))
    x = rng.randn(*dims, cin).astype(np.float32)
    w = (rng.randn(cout, cin, 1, 3, 3) / np.sqrt(cin * 9)).astype(np.float32)
    bias = (0.2 * rng.randn(cout)).astype(np.float32)
    add = rng.randn(dims[0], 2 * dims[1], 2 * dims[2], cout).astype(np.float32)
    up = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, torch.from_numpy(w[:, :, 0]), torch.from_numpy(bias), 1, 1).permute(0, 2, 3, 1).numpy() + add

    def run():
        outs = []
        for rank in range(0, 40, 4):
            monkeypatch.setenv("DR_CONV_RANK", str(rank))
            got = debug_conv(x, w, (1, 1, 1), "up2", None, bias, False, add, False)
            err = np.abs(got - ref).max()
            assert got.shape == ref.shape and err <= 2e-5 * max(1.0, np.abs(ref).max()), f"{name} rank {rank}: max|err| {err:.3e}"
            outs.append(("rank %d" % rank, got))
        return outs
    on_and_off(run, name)


@pytest.mark.parametrize("form", [1, 0])
def test_tail_under_guards(form, parity_hooks):
    """k_tail_m / k_tail against torch (tests/test_tail_gpu.py, its bound), the output starting as poison."""
    from tandem_amd.dr_mvsnet import debug_tail
    from test_tail_gpu import reference
    cases = []
    for D, h, w, qy in ((4, 12, 28, 0), (4, 12, 28, 8), (2, 2, 2, 8)):
        rng = np.random.RandomState(D * 1000 + h * 10 + w + qy)
        x = rng.standard_normal((D // 2, h // 2, w // 2, 16)).astype(np.float32)
        skip = rng.standard_normal((D, h, w, 8)).astype(np.float32)
        wd = (rng.standard_normal((16, 8, 3, 3, 3)) * 0.15).astype(np.float32)
        wp = (rng.standard_normal((1, 8, 3, 3, 3)) * 0.2).astype(np.float32)
        scale = (0.5 + rng.rand(8)).astype(np.float32)
        bias = (rng.standard_normal(8) * 0.3).astype(np.float32)
        cases.append(((x, skip, wd, scale, bias, wp), qy, reference(x, skip, wd, scale, bias, wp)))

    def run():
        outs = []
        for args, qy, ref in cases:
            out = debug_tail(*args, qy=qy, zchunk=0, form=form)
            err = np.abs(out - ref).max()
            assert err <= 2e-5 * np.abs(ref).max(), f"max err {err} of range {np.abs(ref).max()} (form {form}, qy {qy}, shape {ref.shape})"
            outs.append(("%s qy %d" % (ref.shape, qy), out))
        return outs
    on_and_off(run, "tail form %d" % form)


# ------------------------------------------------------------------ c. the DrMvsnet engine
from test_mvs_stages_gpu import _model, _run  # noqa: E402

# id, H, W, views, pose, model, environment
STAGE_CASES = [
    ("trained-64x96-v4-scene", 64, 96, 4, "scene", "trained", {}),
    ("d4-96x64-v4-behind", 96, 64, 4, "behind", (48, 4, 4), {}),
    ("plain-64x96-v4-narrow", 64, 96, 4, "narrow", "plain", {}),
    ("trained-96x64-v2-narrow-z8", 96, 64, 2, "narrow", "trained", dict(DR_PROB_ZCHUNK="8")),
    ("trained-64x96-v4-behind-dchunk8", 64, 96, 4, "behind", "trained", dict(DR_CV_DCHUNK1="8", DR_CV_DCHUNK2="8", DR_CV_DCHUNK3="8")),
]


@pytest.mark.parametrize("case", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_engine_stage_tensors_under_guards(case, trained_blob, tmp_path, monkeypatch, parity_hooks):
    """feat / volume / s*.conv11 / logits / depth / conf of all three stages: the values are held to float64 by tests/test_mvs_stages_gpu.py;
    here every engine tensor, plan upload and scratch buffer is guarded and starts as NaN."""
    tag, H, W, V, pose, model, env = case
    for k in ["DR_PROB_ZCHUNK"] + ["DR_CV_DCHUNK%d" % s for s in (1, 2, 3)]:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob, meta, tens = _model(model, trained_blob, tmp_path)
    win = R.make_case(H, W, V, pose)
    kerns = []

    def run():
        T, kern = _run(blob, win, H, W, V)
        kerns.append(kern)
        return sorted(T.items())
    on_and_off(run, tag)
    assert kerns[0] == kerns[1], "guards changed the kernels the forward ran"
    if "DR_PROB_ZCHUNK" in env:
        assert kerns[0]["s3.prob"] == "k_prob2_regress<8>", kerns[0]
    if "DR_CV_DCHUNK1" in env:
        assert kerns[0]["s1.costvol"] == "k_costvol5<32,8>", kerns[0]


def _window_outputs(m, out):
    return [(n, getattr(out, n).copy()) for n in ("depth", "confidence", "depth_dense", "confidence_dense")] + [("edge", m.tensor("edge").copy())]


def test_engine_window_under_guards(trained_blob, parity_hooks):
    """CallAsync / GetResult at 64x96x3, discard 2.5 and 37.5 (the edge filter's radix select: histograms, scan state), and the same window
    twice on one engine: plan reuse, march flags and histograms are what the first call left, not fresh poison."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    win = scene.make_window(64, 96, 3, seed=2)

    def run():
        outs = []
        for discard in (2.5, 37.5):
            m = DrMvsnet(trained_blob)
            for rep in range(2):
                m.CallAsync(64, 96, 3, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, discard)
                outs += [("discard %g call %d %s" % (discard, rep, n), a) for n, a in _window_outputs(m, m.GetResult())]
            m.close()
        return outs
    outs = on_and_off(run, "window")
    for i in range(0, len(outs), 10):  # the second answer of an engine equals its first
        for (na, a), (nb, b) in zip(outs[i:i + 5], outs[i + 5:i + 10]):
            assert_same_bits(b, a, nb + " against " + na)
    assert (outs[0][1] == 0).mean() < (outs[10][1] == 0).mean()  # (37.5 % discards more than 2.5 %)


def test_engine_feature_cache_and_resolution_change_under_guards(trained_blob, parity_hooks):
    """set_feature_cache(4) over three sliding 3-view windows at 64x96 (the single-view FeatureNet plan, cache entries, the device compare),
    then 96x64 on the same engine: release() frees every tensor under guards, so the check at free runs."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet

    def run():
        outs = []
        m = DrMvsnet(trained_blob)
        m.set_feature_cache(4)
        for H, W in ((64, 96), (96, 64)):
            big = scene.make_window(H, W, 5, seed=31)
            for k in range(3):
                bgrs = [np.ascontiguousarray(b) for b in big["bgrs"][k:k + 3]]
                m.CallAsync(H, W, 3, 1, bgrs, big["K"], list(big["c2ws"][k:k + 3]), 0.5, 5.0, 10.0)
                outs += [("%dx%d window %d %s" % (H, W, k, n), a) for n, a in _window_outputs(m, m.GetResult())]
        st = m.feature_cache_stats()
        assert st["single_view_plan"] and st["batch_windows"] == 2 and st["views_from_cache"] == 8, st
        m.close()
        return outs
    on_and_off(run, "feature cache")


# ------------------------------------------------------------------ c2. what an engine leaves behind
def _live():
    """Guarded buffers alive right now (dr_guard_check), none of them written outside."""
    st, rep = check()
    assert st["violations"] == 0, rep
    return st["live"]


def test_a_plan_that_fails_half_way_leaves_nothing_behind(tmp_path, parity_hooks):
    """depth_num = (16, 12, 4): stage 2's 12 planes are refused (DR_ERR_UNSUPPORTED) after FeatureNet and stage 1 have been allocated.
    The engine then holds what it held before the call, and nothing once it is closed."""
    from synth import scene
    from tandem_amd import _lib
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    blob = str(tmp_path / "d12.tdmw")
    Wt.write_blob(blob, Wt.random_state((16, 12, 4)), depth_num=(16, 12, 4))
    win = scene.make_window(64, 96, 3, seed=2)
    with guarded():
        before = _live()
        m = DrMvsnet(blob)
        created = _live()
        assert created > before  # (the engine's own constants: the count does see this library's allocations)
        with pytest.raises(_lib.DrError) as e:
            m.CallAsync(64, 96, 3, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
        assert e.value.code == 6 and "depth_num[1]=12" in str(e.value), e.value
        assert _live() == created
        m.close(force=True)
        assert _live() == before


def test_a_full_engine_life_cycle_returns_every_buffer(trained_blob, parity_hooks):
    """Window, feature cache on (re-plan with the single-view plan and its entries), two sliding windows, another window shape (re-plan),
    autotune (re-planned candidates in the plan's arena), profile (its events), close."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    big = scene.make_window(64, 96, 5, seed=31)
    win5 = scene.make_window(96, 128, 5, seed=7)

    def call(m, H, W, w, views):
        bgrs = [np.ascontiguousarray(w["bgrs"][v]) for v in views]
        m.CallAsync(H, W, len(views), 1, bgrs, w["K"], [w["c2ws"][v] for v in views], 0.5, 5.0, 10.0)
        assert_no_nan(m.GetResult().depth, "%dx%d views %s" % (H, W, list(views)))
    with guarded():
        before = _live()
        m = DrMvsnet(trained_blob)
        call(m, 64, 96, big, range(0, 3))
        one_plan = _live()
        m.set_feature_cache(4)
        assert _live() > one_plan  # (the entries and the single-view tensors)
        call(m, 64, 96, big, range(1, 4))
        call(m, 64, 96, big, range(2, 5))
        st = m.feature_cache_stats()
        assert st["single_view_plan"] and st["views_from_cache"] == 2, st
        call(m, 96, 128, win5, range(5))
        m.autotune(2)
        assert len(m.profile()) > 40
        m.close(force=True)
        assert _live() == before


# ------------------------------------------------------------------ e. the tracker
import test_tracker_gpu as TT  # noqa: E402


@pytest.mark.parametrize("frac", [0.05, 0.0])
def test_tracker_calc_res_and_calc_g_under_guards(frac, parity_hooks):
    H, W = 96, 128
    p = TT.pair(H, W, H + int(100 * frac), frac)
    aff_ref, aff_new = [0.02, 1.5], [-0.01, -0.7]

    def run():
        g, o = TT.both(p)
        outs = []
        for t in (g, o):
            t.setReference(p["pc_u"], p["pc_v"], p["pc_idepth"], p["pc_color"], 1.3, aff_ref)
            t.setNew(p["dI_new"])
        for i, T in enumerate((p["refToNew"], np.eye(4))):
            out_g, sums_g = g.calcRes(T, 0.9, aff_new, 20.0, return_sums=True)
            out_o, sums_o = o.calcRes(T, 0.9, aff_new, 20.0)
            for k, (a, b) in enumerate(zip(g.warped(), o.warped())):
                assert np.array_equal(TT.bits(a), TT.bits(b)), f"warped[{k}] differs at {(TT.bits(a) != TT.bits(b)).sum()} of {len(a)} points"
                outs.append(("T%d warped[%d]" % (i, k), np.ascontiguousarray(a, np.float32)))
            assert np.allclose(sums_g, sums_o, rtol=TT.SUM_RTOL, atol=0), (sums_g, sums_o)
            Hg, bg, rg = g.calcG(0.9, aff_new, return_raw=True)
            Ho, bo, ro = o.calcG(0.9, aff_new)
            if sums_o[2] > 0:
                assert np.allclose(rg, ro, rtol=TT.SUM_RTOL, atol=1e-9 * np.abs(ro).max())
            outs += [("T%d sums" % i, np.asarray(sums_g, np.float64).view(np.uint8)), ("T%d G" % i, np.asarray(rg, np.float64).view(np.uint8))]
            assert not np.isnan(np.asarray(sums_g, np.float64)).any() and not np.isnan(np.asarray(rg, np.float64)).any()
        g.close()
        return outs
    on_and_off(run, "tracker frac %g" % frac)


@pytest.mark.parametrize("H,W,step", [(96, 128, 1), (96, 128, 3), (120, 160, 1)])
def test_tracker_append_dense_reference_under_guards(H, W, step, parity_hooks):
    """The hand-off with n_max exactly the resulting point count -- the last point k_trk_row_write stores is the last element of the point
    arrays, their back guard starts behind it -- and with one less: DR_ERR_CAPACITY and nothing written."""
    from tandem_amd import _lib
    p = TT.pair(H, W, 11 + step, 0.03)
    K = np.array([[p["fx"], 0, p["cx"]], [0, p["fy"], p["cy"]], [0, 0, 1]], np.float32)
    Ki = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    T = np.linalg.inv(p["c2w_ref"]) @ p["c2w_new"]
    KRKi = (K @ T[:3, :3].astype(np.float32)) @ Ki
    Kt = K @ T[:3, 3].astype(np.float32)
    depth = p["depth_new"].copy()
    depth[::7, ::5] = 0.0
    # the oracle once, with room to spare: the count and the lists every run is compared with
    from oracle.tracker_oracle import TrackerOracle
    o = TrackerOracle(W, H, 9.0, 20.0, H * W)
    o.setK(p["fx"], p["fy"], p["cx"], p["cy"])
    o.setReference(p["pc_u"], p["pc_v"], p["pc_idepth"], p["pc_color"], 1.0, [0, 0])
    n_o, proj_o = o.appendDenseReference(depth, KRKi, Kt, step, True, None, p["dI_ref"])
    want = [np.ascontiguousarray(a, np.float32).copy() for a in o.points()]
    n_sparse = len(p["pc_u"])
    assert n_o > n_sparse + 300

    def run():
        from tandem_amd.dr_tracker import DrCoarseTracker
        outs = []
        for n_max in (n_o, n_o - 1):
            g = DrCoarseTracker(W, H, 9.0, 20.0)
            g.setK(W, H, p["fx"], p["fy"], p["cx"], p["cy"])
            g.init(n_max)
            g.setReference(p["pc_u"], p["pc_v"], p["pc_idepth"], p["pc_color"], 1.0, [0, 0])
            before = [np.ascontiguousarray(a, np.float32).copy() for a in g.points()]
            if n_max == n_o:
                assert g.appendDenseReference(depth, KRKi, Kt, step, True, None, p["dI_ref"]) == n_o
                assert np.array_equal(TT.bits(g.zbuffer()), TT.bits(proj_o))
                for k, (a, b) in enumerate(zip(g.points(), want)):
                    assert np.array_equal(TT.bits(a), TT.bits(b)), f"point array {k} differs"
                outs.append(("zbuffer", np.ascontiguousarray(g.zbuffer(), np.float32)))
            else:
                with pytest.raises(_lib.DrError) as e:
                    g.appendDenseReference(depth, KRKi, Kt, step, True, None, p["dI_ref"])
                assert e.value.code == 5
                assert len(g.points()[0]) == n_sparse  # nothing was appended
                for k, (a, b) in enumerate(zip(g.points(), before)):
                    assert np.array_equal(TT.bits(a), TT.bits(b)), f"sparse point array {k} changed"
            outs += [("n_max %d points[%d]" % (n_max, k), np.ascontiguousarray(a, np.float32)) for k, a in enumerate(g.points())]
            g.close()
        return outs
    on_and_off(run, "append %dx%d step %d" % (H, W, step))


def test_a_tracker_life_cycle_returns_every_buffer(parity_hooks):
    """init, one reference, the dense hand-off (its lazily allocated group), one calcRes / calcG under the timing events, close."""
    from tandem_amd.dr_tracker import DrCoarseTracker
    H, W = 96, 128
    p = TT.pair(H, W, 5, 0.03)
    K = np.array([[p["fx"], 0, p["cx"]], [0, p["fy"], p["cy"]], [0, 0, 1]], np.float32)
    T = np.linalg.inv(p["c2w_ref"]) @ p["c2w_new"]
    KRKi = (K @ T[:3, :3].astype(np.float32)) @ np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    with guarded():
        before = _live()
        g = DrCoarseTracker(W, H, 9.0, 20.0)
        g.setK(W, H, p["fx"], p["fy"], p["cx"], p["cy"])
        g.init(H * W)
        g.setReference(p["pc_u"], p["pc_v"], p["pc_idepth"], p["pc_color"], 1.0, [0, 0])
        assert g.appendDenseReference(p["depth_new"], KRKi, K @ T[:3, 3].astype(np.float32), 2, True, None, p["dI_ref"]) > len(p["pc_u"])
        g.setNew(p["dI_new"])
        g.startTiming()
        out = g.calcRes(p["refToNew"], 1.0, [0, 0], 20.0)
        g.calcG(1.0, [0, 0])
        assert g.endTimingMilliseconds() > 0 and np.isfinite(out[0])
        assert _live() > before
        g.close()
        assert _live() == before


# ------------------------------------------------------------------ d. DrFusion
import fusion_helpers as FH  # noqa: E402


def _fusion(opt):
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions
    return DrFusion(DrFusionOptions(**opt))


def _blocks_as_arrays(tag, blocks):
    keys = sorted(blocks)
    return [(tag + " keys", np.array(keys, np.int32).reshape(-1, 3).view(np.uint8)), (tag + " voxels", np.stack([blocks[k] for k in keys]).view(np.uint8))]


def _oracle_record(opt, scans, views):
    """The oracle's answers, computed once per test: per scan the ray-cast at views[i] and the update count; the final blocks."""
    from oracle.tsdf_oracle import TsdfOracle
    o, rec = TsdfOracle(**opt), []
    for (bgr, depth, pose), view in zip(scans, views):
        assert o.integrate(bgr, depth, pose) == 0
        rec.append((o.render(view), o.stats()["updated_last"]))
    return o, rec


def _engine_against_record(opt, scans, views, rec, tag):
    """A new engine through the scans: every ray-cast and update count as recorded.  Returns the engine and its renders."""
    f, outs = _fusion(opt), []
    for i, ((bgr, depth, pose), view) in enumerate(zip(scans, views)):
        f.IntegrateScanAsync(bgr, depth, pose)
        f.RenderAsync([view])
        rb, rd = f.GetRenderResult()
        (ob, od), upd = rec[i]
        assert np.array_equal(rd[0].view(np.uint32), od.view(np.uint32)), f"{tag} scan {i}: ray-cast depth differs at {(rd[0] != od).sum()} px"
        assert np.array_equal(rb[0], ob), f"{tag} scan {i}: ray-cast colour differs"
        assert f.stats()["updated_last"] == upd
        outs += [("%s depth %d" % (tag, i), rd[0].copy()), ("%s bgr %d" % (tag, i), rb[0].copy())]
    return f, outs


def test_fusion_integrate_raycast_export_under_guards(parity_hooks):
    """(64, 64, 0.04, 6) of test_fusion_gpu.py::test_integrate_and_raycast_bit_exact: voxel pool, hash tables, visible lists, render buffers."""
    from synth import scene
    from test_fusion_gpu import assert_same_volume
    H, W, vs, n = 64, 64, 0.04, 6
    sc = scene.make_scans(n, H, W, seed=H + n)
    opt = FH.options(sc, H, W, vs)
    views = [sc["scans"][(i + 1) % n][2] for i in range(n)]
    o, rec = _oracle_record(opt, sc["scans"], views)

    def run():
        f, outs = _engine_against_record(opt, sc["scans"], views, rec, "64x64")
        assert_same_volume(f, o)
        outs += _blocks_as_arrays("export", f.export_blocks())
        f.close()
        return outs
    on_and_off(run, "integrate + ray-cast")


def test_fusion_blocks_outside_the_dense_grid_under_guards(parity_hooks):
    """test_fusion_gpu.py::test_blocks_outside_the_dense_grid's scene, two scans: the open-addressing table beside the dense grid."""
    from synth import scene
    from test_fusion_gpu import assert_same_volume
    H, W, vs = 96, 128, 0.02
    sc = scene.make_scans(2, H, W, seed=6)
    opt = FH.options(sc, H, W, vs)
    S = np.eye(4, dtype=np.float32)
    c, s = np.cos(1.45), np.sin(1.45)
    S[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    S[:3, 3] = (40.2, 0.3, -0.2)
    scans = FH.shifted(sc["scans"], S)
    views = [p for _, _, p in scans]
    o, rec = _oracle_record(opt, scans, views)
    assert (rec[-1][0][1] > 0).mean() > 0.3

    def run():
        f, outs = _engine_against_record(opt, scans, views, rec, "far")
        xs = [k[0] for k in f.export_blocks()]
        assert min(xs) < 256 <= max(xs), (min(xs), max(xs))
        assert_same_volume(f, o)
        outs += _blocks_as_arrays("export", f.export_blocks())
        f.close()
        return outs
    on_and_off(run, "outside the dense grid")


def test_fusion_mesh_and_mesh_update_under_guards(parity_hooks):
    """Marching cubes at (64, 64, 0.04, 4) against the oracle, and one incremental update: baseline after three scans, update after the
    fourth, assembled = the full extraction byte for byte (tests/test_fusion_mesh_update_gpu.py)."""
    from synth import scene
    from tandem_amd.dr_fusion import MeshPatches
    from test_mesh_gpu import assert_same_mesh as same_triangles
    H, W, vs, n = 64, 64, 0.04, 4
    lo, hi = (-2.0, -2.0, 0.0), (2.0, 2.0, 4.0)
    sc = scene.make_scans(n, H, W, seed=H + n)
    opt = FH.options(sc, H, W, vs)
    views = [p for _, _, p in sc["scans"]]
    o, rec = _oracle_record(opt, sc["scans"], views)
    want = o.extract_mesh(lo, hi)
    assert len(want[0]) > 1000

    def run():
        f, _ = _engine_against_record(opt, sc["scans"][:3], views, rec, "mesh")
        m = MeshPatches()
        upd = f.GetMeshUpdate(lo, hi)
        assert upd[0], "the first update is full"
        m.apply(upd)
        FH.assert_same_mesh(m.assemble(), f.GetMesh(lo, hi), "baseline")
        FH.feed(f, *sc["scans"][3])
        upd = f.GetMeshUpdate(lo, hi)
        st = f.mesh_update_stats()
        assert not upd[0] and 0 < st["meshed"] <= st["scope"], st
        m.apply(upd)
        f.ExtractMeshAsync(lo, hi)
        got = f.GetMeshSync()
        assert f.dr_mesh_num == len(want[0])
        same_triangles(got, want)
        FH.assert_same_mesh(m.assemble(), got, "after one update")
        f.close()
        return [("vertices", got[0].copy()), ("colours", got[1].copy()), ("update vertices", np.array(upd[3])), ("update first", np.array(upd[2]).view(np.uint8))]
    on_and_off(run, "mesh")


def test_fusion_streaming_map_scope_under_guards(tmp_path, parity_hooks):
    """Two scans of tests/test_fusion_streaming_gpu.py::test_round_trip_out_and_in_is_exact's scene; everything to the host store; the
    map-scope mesh; then, as tests/test_fusion_render_bands_gpu.py does, the map through a file into the host store of a second streaming
    engine and a map-scope render through a staging too small for one pass, in depth bands: block staging, band plan uploads."""
    from synth import scene
    from tandem_amd import _lib
    from tandem_amd.dr_fusion import MESH_MAP, RENDER_MAP, streaming_min_radius
    from test_fusion_streaming_gpu import ALL_HI, ALL_LO, assert_same_blocks
    H, W = 96, 128
    sc = scene.make_scans(2, H, W, seed=11)
    opt = FH.options(sc, H, W, 0.02)
    views = [p for _, _, p in sc["scans"]]
    o, rec = _oracle_record(opt, sc["scans"], views)
    blocks = o.export_blocks()
    lo, hi = FH.box_of(blocks, 0.02)
    want_mesh = o.extract_mesh(lo, hi)
    pose, (ob, od) = views[-1], rec[-1][0]
    assert (od > 0).mean() > 0.3
    count = [0]

    def run():
        count[0] += 1
        path = str(tmp_path / ("map%d.drfmap" % count[0]))
        f, outs = _engine_against_record(opt, sc["scans"], views, rec, "stream")
        f.set_streaming(streaming_min_radius(f.options))
        f.stream_out_region(ALL_LO, ALL_HI)
        st = f.streaming_stats()
        assert st["resident"] == 0 and st["host"] == len(blocks), st
        assert_same_blocks(f.export_host_blocks(), blocks, "host store")
        f.set_mesh_scope(MESH_MAP)
        got = f.GetMesh(lo, hi)
        assert np.array_equal(FH.canon(*got), FH.canon(*want_mesh)), "map-scope mesh against the oracle"
        assert f.mesh_stats()[1] > 0
        f.save_map(path)
        f.close()
        g = _fusion(opt)
        g.set_streaming(streaming_min_radius(g.options))
        g.load_map(path)
        st = g.streaming_stats()
        assert st["resident"] == 0 and st["host"] == len(blocks), st
        g.set_render_scope(RENDER_MAP, 0)
        g.set_render_bands(0)
        g.RenderAsync([pose])
        rb, rd = g.GetRenderResult()
        assert np.array_equal(rd[0].view(np.uint32), od.view(np.uint32)) and np.array_equal(rb[0], ob), "map-scope render against the oracle"
        n = g.render_stats()[0]
        assert n > 0 and g.render_band_stats() == (1, n, n, 0)
        g.set_render_bands(8)
        for frac in (0.55, 0.65, 0.75, 0.85, 0.95):  # the largest staging below the union that the band planner can serve
            cap = int(n * frac)
            g.set_render_scope(RENDER_MAP, cap)
            try:
                g.RenderAsync([pose])
                break
            except _lib.DrError as e:
                assert e.code == 5
        else:
            raise AssertionError("no staging below the %d blocks of this pose is served in 8 bands" % n)
        bb, bd = g.GetRenderResult()
        bands = g.render_band_stats()
        print("union %d blocks, staging %d, bands %s" % (n, cap, bands))
        assert bands[0] >= 2 and bands[1] <= cap < n and bands[3] == 1, (bands, cap, n)
        assert np.array_equal(bd[0].view(np.uint32), od.view(np.uint32)) and np.array_equal(bb[0], ob), "banded map-scope render against the oracle"
        assert_same_blocks(g.export_all_blocks(), blocks, "nothing changed")
        assert g.streaming_stats()["resident"] == 0, "no block moved"
        outs += [("mesh vertices", got[0].copy()), ("mesh colours", got[1].copy()), ("map file", np.frombuffer(open(path, "rb").read(), np.uint8)),
                 ("depth", rd[0].copy()), ("bgr", rb[0].copy()), ("banded depth", bd[0].copy()), ("banded bgr", bb[0].copy())]
        g.close()
        return outs
    on_and_off(run, "streaming")


def test_fusion_save_load_merge_under_guards(tmp_path, parity_hooks):
    """Map A = scans 0, 1 and map B = scans 2, 3 of one scene: save both, load A into a new engine (equal blocks), merge B's file into it:
    the merged map equals tests/test_map_merge.py's restatement, and its file the restatement's bytes."""
    from synth import scene
    from test_fusion_map_file_gpu import file_blocks
    from test_fusion_map_merge_gpu import compose_map
    from test_fusion_streaming_gpu import assert_same_blocks
    from test_map_merge import np_merge_maps
    H, W = 96, 128
    sc = scene.make_scans(4, H, W, seed=11)
    opt = FH.options(sc, H, W, 0.02)
    want = {}

    def run():
        tag = "on" if not want.get("ran") else "off"
        want["ran"] = True
        FA, FB, FM = (str(tmp_path / (n + tag + ".drfmap")) for n in "ABM")
        for path, idx in ((FA, (0, 1)), (FB, (2, 3))):
            U = _fusion(FH.unbounded(opt))
            for i in idx:
                FH.feed(U, *sc["scans"][i])
            U.save_map(path)
            U.close()
        A, B = file_blocks(FA)[0], file_blocks(FB)[0]
        if "merged" not in want:
            want["merged"], want["st"] = np_merge_maps(A, B, 64)
            assert min(want["st"]["added"], want["st"]["combined"], want["st"]["averaged"]) > 0, want["st"]
        f = _fusion(opt)
        f.load_map(FA)
        assert_same_blocks(f.export_blocks(), A, "loaded")
        f.merge_map(FB, 64)
        got = f.export_blocks()
        assert_same_blocks(got, want["merged"], "merged")
        f.save_map(FM, 5)
        f.close()
        data = open(FM, "rb").read()
        assert data == compose_map(want["merged"]), "the merged map's file"
        return [("file A", np.frombuffer(open(FA, "rb").read(), np.uint8)), ("file B", np.frombuffer(open(FB, "rb").read(), np.uint8)),
                ("merged file", np.frombuffer(data, np.uint8))]
    on_and_off(run, "save / load / merge")


def test_fusion_transform_and_align_under_guards(tmp_path, parity_hooks):
    """drf_transform_map, drf_align_system and drf_align_map on the random pair of tests/test_map_align.py (40 source blocks) and
    drf_align_system at 65 source blocks (one more than a grid / fold boundary): the per-call device scratch (Held) under guards."""
    from test_fusion_map_file_gpu import engine
    from test_fusion_map_transform_gpu import options, write
    from test_fusion_map_align_gpu import result_dict
    from test_map_align import SMALL, T37, VS, assert_same_result, assert_same_system, np_align_maps, np_align_system, random_pair
    from test_map_transform import np_transform_map
    src, ref = random_pair(3)
    src65, ref65 = random_pair(10 + 65, n_src=65)
    paths = {n: str(tmp_path / (n + ".drfmap")) for n in ("src", "ref", "src65", "ref65", "want")}
    for n, m in (("src", src), ("ref", ref), ("src65", src65), ("ref65", ref65)):
        write(paths[n], VS, *m)
    wc, wv, st = np_transform_map(src[0], src[1], T37, VS)
    want_file = write(paths["want"], VS, wc, wv)
    assert st["blocks"] > 0 and st["voxels"] > 0
    want_sys, want_sys65 = np_align_system(src, ref, SMALL, VS), np_align_system(src65, ref65, SMALL, VS)
    assert want_sys[1][1] > 0 and want_sys65[1][1] > 0
    opt_align = dict(max_iters=2, min_valid=0.01)
    want_align = np_align_maps(src, ref, SMALL, VS, **opt_align)
    want_align.pop("trace", None)
    count = [0]

    def run():
        count[0] += 1
        out = str(tmp_path / ("out%d.drfmap" % count[0]))
        f = engine(options())
        f.transform_map(paths["src"], T37, out, 5)
        got_file = open(out, "rb").read()
        assert got_file == want_file, "transform_map against the restatement"
        assert f.transform_stats()[2:5] == (st["blocks"], st["voxels"], st["refused"])
        got = f.align_system(paths["src"], paths["ref"], SMALL)
        assert_same_system(got, want_sys, "align_system, 40 blocks")
        got65 = f.align_system(paths["src65"], paths["ref65"], SMALL)
        assert_same_system(got65, want_sys65, "align_system, 65 blocks")
        r = f.align_map(paths["src"], paths["ref"], SMALL, raise_on_failure=False, **opt_align)
        assert_same_result(result_dict(r), want_align, "align_map")
        f.close()
        return [("transformed file", np.frombuffer(got_file, np.uint8)), ("system", np.asarray(got[0], np.float64).view(np.uint8)),
                ("system 65", np.asarray(got65[0], np.float64).view(np.uint8)), ("pose", np.asarray(r.T, np.float64).view(np.uint8)),
                ("sums", np.asarray(r.sums, np.float64).view(np.uint8))]
    on_and_off(run, "transform / align")


def test_fusion_combine_under_guards(parity_hooks):
    """drf_test_combine on 65536 pairs (every colour pair at weight 7) against the oracle's table, as test_combine_exhaustive_... does."""
    from oracle import tsdf_oracle
    from synth import scene
    sc = scene.make_scans(1, 8, 8)
    opt = FH.options(sc, 8, 8, 0.02, num_blocks=64, num_buckets=64)
    O = tsdf_oracle.lib()
    O.tsdf_pin_combine_colour_table.argtypes = [C.c_ubyte, C.c_void_p]
    c, vc = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    a = np.zeros((65536, 8), np.uint8)
    b = np.zeros((65536, 8), np.uint8)
    a[:, 4] = a[:, 5] = a[:, 6] = c.ravel()
    b[:, 4] = b[:, 5] = b[:, 6] = vc.ravel()
    a[:, 7], b[:, 7] = 7, 1
    want = np.empty(65536, np.uint8)
    O.tsdf_pin_combine_colour_table(7, want.ctypes.data)

    def run():
        f = _fusion(opt)
        got = f.test_combine(a, b, 255)
        f.close()
        for ch in (4, 5, 6):
            assert np.array_equal(got[:, ch], want), f"{np.count_nonzero(got[:, ch] != want)} colour blends differ from the restatement"
        assert (got[:, 7] == 8).all()
        return [("combined", got)]
    on_and_off(run, "combine")
