"""-m gpu: every layer INSIDE the engine -- FeatureNet's trunk and heads, CostRegNet's ten layers per stage -- against a float64 restatement of that ONE
layer (tests/mvs_stage_ref.py, "THE LAYER RESTATEMENTS"), fed the engine's own input tensor(s) and compared per element.  tests/test_conv_gpu.py checks
the convolution kernel families on their own (drm_debug_conv) and tests/test_mvs_stages_gpu.py the stage tensors; between the two, the layers of the plan
the engine really builds -- the skip operands, the padded tensors, the tuned plans of conv_tuned.h, which match two exact shapes only -- were covered by the
whole-window bounds alone.  Here:

  * the layer list is DRIVEN BY THE PROFILE: every op named fn.* or s<S>.conv* must map to a tensor that was checked (where a fused kernel leaves no
    tensor the restatement spans the layers up to the next one that exists: fn.front -> fn.conv0.1, fn.head3 -> feat3), and every layer the model has
    must have been produced by some op: none is left out;
  * the bound is CONV_BOUND = 2e-5 of layer_scale() = max(max |value before the ReLU|, max |output|) of the float64 layer; the fp32 oracle's own layers sit
    at E_LAYER of it (tests/test_mvs_stage_ref.py asserts 4 E_LAYER <= CONV_BOUND): a margin over the reference, not a fit to the kernels;
  * the zero border of the padded feat1..3 is read back through device_tensor + dr_memcpy_d2h and must still be zero bits after the forward;
  * the shapes: the six smallest windows the engine accepts (mvs_stage_ref.SMALL_WINDOWS: 32-pixel sides, half of k_fn_front's / k_fn_head3's 64-pixel tile,
    k_prob2's 64-column tile at w = 8, CostRegNet levels of (6, 1, 1) and (1, 4, 4)) with the trained blob, 48/4/4, 16/8/8 and the plain-variance model, two
    of them with DR_PROB_ZCHUNK 3 and 8 -- on these the stage tensors are checked too (test_mvs_stages_gpu._check_stages); one window of ordinary size (64 x 96
    x 4) to tell "small" from "wrong"; small windows with one kernel family preferred (DR_CONV_MARCH / ROWMARCH / WINO = 2, DR_CONV_ASYNC = 1), so that every
    family the tuned plans run also runs in the engine at a small window; and the two shapes conv_tuned.h has rows for, 480 x 640 x 7 (48/32/8) and 320 x 512 x 7
    (48/4/4), with the tuned rows and with DR_CONV_NO_TUNED=1 -- no smaller window reaches a row, so for those plans the headline shape IS the smallest one.
    A tuned case costs one forward plus the downloads on the GPU and about 15 s of float64 convolutions on the host (printed per case).

Measured on an MI355X: DESIGN.md section 4 has the table (largest share of the bound per case, the applied tuned rows, the families)."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import mvs_stage_ref as R
from test_mvs_stages_gpu import _check_stages, _model

pytestmark = pytest.mark.gpu

SWITCHES = ("DR_PROB_ZCHUNK", "DR_CV_DCHUNK1", "DR_CV_DCHUNK2", "DR_CV_DCHUNK3", "DR_CONV_MARCH", "DR_CONV_ROWMARCH", "DR_CONV_WINO", "DR_CONV_ASYNC",
            "DR_CONV_NO_TUNED", "DR_CONV_RANK")

# id, H, W, views, pose, model, environment
SMALL_CASES = [
    ("trained-32x32-v2-scene", 32, 32, 2, "scene", "trained", {}),
    ("d4-32x32-v4-behind", 32, 32, 4, "behind", (48, 4, 4), {}),
    ("generic-32x64-v3-rotated-z8", 32, 64, 3, "rotated", (16, 8, 8), {"DR_PROB_ZCHUNK": "8"}),
    ("trained-64x32-v8-narrow-z3", 64, 32, 8, "narrow", "trained", {"DR_PROB_ZCHUNK": "3"}),
    ("d4-32x96-v3-rotated", 32, 96, 3, "rotated", (48, 4, 4), {}),
    ("plain-96x32-v2-behind", 96, 32, 2, "behind", "plain", {}),
    ("trained-96x32-v2-behind", 96, 32, 2, "behind", "trained", {}),
]
# one kernel family preferred wherever the planner lets it apply (k_conv_a: DR_CONV_ASYNC=1 plans it alone and falls back to k_conv where no plan fits)
FORCED_CASES = [
    ("trained-32x64-v3-rotated-march", 32, 64, 3, "rotated", "trained", {"DR_CONV_MARCH": "2"}),
    ("d4-32x32-v4-behind-rowmarch", 32, 32, 4, "behind", (48, 4, 4), {"DR_CONV_ROWMARCH": "2"}),
    ("trained-64x32-v8-narrow-wino", 64, 32, 8, "narrow", "trained", {"DR_CONV_WINO": "2"}),
    ("trained-32x96-v3-rotated-async", 32, 96, 3, "rotated", "trained", {"DR_CONV_ASYNC": "1"}),
]
ORDINARY_CASES = [("trained-64x96-v4-scene", 64, 96, 4, "scene", "trained", {})]
TUNED_SHAPES = {"480x640": (480, 640, 7, "scene", "trained"), "320x512": (320, 512, 7, "scene", (48, 4, 4))}
TUNED_CASES = [("tuned-%s-v7%s" % (k, "-notuned" if env else ""),) + v + (env,) for k, v in TUNED_SHAPES.items() for env in ({}, {"DR_CONV_NO_TUNED": "1"})]

# families the default plans of the tuned shapes run that the planner rightly refuses at EVERY small shape: {family: the rule of plan_conv that refuses it}
REFUSED_AT_SMALL_SHAPES = {}

# ops that leave no tensor of their own name: the tensor they (help to) produce
FUSED_OPS = {"fn.front": "fn.conv0.1", "fn.out1": "feat1", "fn.skip2": "inter2", "fn.out2": "feat2", "fn.head3": "feat3", "fn.out3a": "feat3",
             "fn.out3b": "feat3", "fn.out3c": "feat3", "fn.out3d": "feat3"}
_PROFILES = {}  # case id -> {op: kernel} of the cases this session has run


def _is_layer_op(op):
    return op.startswith("fn.") or re.match(r"s\d\.conv", op) is not None


def _tensor_of(op, layers):
    """The checked tensor an op writes: its own name, a fused op's target, or -- a layer planned as several launches, `<layer>.<index>` -- the layer's."""
    if op in FUSED_OPS:
        return FUSED_OPS[op]
    if op in layers:
        return op
    base = op.rsplit(".", 1)[0]
    return base if base in layers and op.rsplit(".", 1)[1].isdigit() else None


def family(kernel):
    return kernel.split("<")[0]


def _set_switches(mp, env):
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def _start(case, trained_blob, tmp_path):
    """upload, forward(1), profile(): the engine (still open: its tensors are read one at a time), the profile rows and the model."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    tag, H, W, V, pose, model, _ = case
    blob, meta, tens = _model(model, trained_blob, tmp_path)
    win = R.make_case(H, W, V, pose)
    m = DrMvsnet(blob)
    m.upload(H, W, V, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), win["depth_min"], win["depth_max"], 2.5)
    m.forward(1)
    prof = m.profile()
    _PROFILES[tag] = {r["op"]: r["kernel"] for r in prof}
    return m, prof, win, meta, tens


def _profile_of(case, trained_blob, tmp_path, monkeypatch):
    """{op: kernel} of a case: from the run this session already made, else from a run of its own (no tensor is downloaded)."""
    if case[0] not in _PROFILES:
        with monkeypatch.context() as mp:
            _set_switches(mp, case[6])
            _start(case, trained_blob, tmp_path)[0].close()
    return _PROFILES[case[0]]


def _check_layers(tag, m, prof, win, meta, tens):
    """Every layer of the plan against its float64 restatement, fed the engine's own input.  Prints one line per layer (kernels, share of the bound, the
    worst element); returns (violations, (largest share, its layer))."""
    layers = R.all_layers(meta)
    by_name = {l.name: l for l in layers}
    kernels, unmatched = {}, []
    for r in prof:
        if _is_layer_op(r["op"]):
            t = _tensor_of(r["op"], by_name)
            if t is None:
                unmatched.append(r["op"])
            else:
                kernels.setdefault(t, []).append(r["kernel"])
    bad = []
    if unmatched:
        bad.append("ops matched to no checked tensor: %s" % unmatched)
    if set(by_name) - set(kernels):
        bad.append("layers no op of the profile produces: %s" % sorted(set(by_name) - set(kernels)))
    # tensors are downloaded when first needed and dropped after their last use (at 480 x 640 x 7 all of them together are 1.5 GB as float32)
    uses = {}
    for l in layers:
        for n in l.inputs + (l.name,):
            uses[n] = uses.get(n, 0) + 1
    held = {}

    def take(n):
        if n not in held:
            held[n] = R.image64(win["bgrs"], win["ref_index"]) if n == "images" else m.tensor(n)
        a = held[n]
        uses[n] -= 1
        if not uses[n]:
            del held[n]
        return a

    worst = (0.0, None)
    for l in layers:
        if l.name not in kernels:
            for n in l.inputs + (l.name,):
                uses[n] -= 1
            continue
        out, pre = l.fn(*[take(n) for n in l.inputs], tens)
        got = take(l.name)
        if got.shape != out.shape:
            bad.append("%s: shape %s, the layer's is %s" % (l.name, got.shape, out.shape))
            continue
        err = np.abs(got - out)
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(np.where(np.isfinite(err), err, np.inf))), err.shape))
        share = float(err[at]) / (R.CONV_BOUND * R.layer_scale(out, pre))
        print("%s %-11s %-44s %.3f of the bound at %s of %s" % (tag, l.name, " + ".join(kernels[l.name]), share, at, out.shape))
        if not share <= 1.0:  # (NaN fails)
            bad.append("%s (%s): %.3f of the bound at %s" % (l.name, " + ".join(kernels[l.name]), share, at))
        if not share <= worst[0]:
            worst = (share, l.name)
    print("%s LARGEST SHARE %.3f of the bound (%s); %d ops on %d tensors, none left out: %s" % (tag, worst[0], worst[1], sum(len(v) for v in kernels.values()),
                                                                                             len(kernels), not unmatched))
    return bad, worst


def _check_feat_borders(tag, m):
    """feat1..3 carry a one-pixel zero border that is written once, when the tensor is allocated: producers only touch the interior.  The raw allocation
    (device_tensor + dr_memcpy_d2h) must still have zero BITS there after the forward, and its interior must be what tensor() hands out."""
    from tandem_amd import _lib
    bad = []
    for s in (1, 2, 3):
        name = "feat%d" % s
        logical = m.tensor(name)
        V, h, w, c = logical.shape
        ptr, n = m.device_tensor(name)
        if n != V * (h + 2) * (w + 2) * c:
            bad.append("%s: %d floats in memory, a one-pixel border would make %d" % (name, n, V * (h + 2) * (w + 2) * c))
            continue
        raw = np.empty(n, np.float32)
        _lib.check(_lib.lib().dr_memcpy_d2h(raw.ctypes.data_as(C.c_void_p), ptr, n * 4))
        raw = raw.reshape(V, h + 2, w + 2, c)
        bits = raw.view(np.uint32)
        dirty = int(np.count_nonzero(bits[:, 0]) + np.count_nonzero(bits[:, -1]) + np.count_nonzero(bits[:, 1:-1, 0]) + np.count_nonzero(bits[:, 1:-1, -1]))
        print("%s %s border: %d of %d words non-zero" % (tag, name, dirty, V * c * (2 * (w + 2) + 2 * h)))
        if dirty:
            bad.append("%s: %d border words overwritten" % (name, dirty))
        if not np.array_equal(raw[:, 1:-1, 1:-1].view(np.uint32), logical.view(np.uint32)):
            bad.append("%s: the interior of the raw tensor is not what tensor() returns" % name)
    return bad


def _run_case(case, trained_blob, tmp_path, monkeypatch, stages):
    tag, H, W, V = case[:4]
    _set_switches(monkeypatch, case[6])
    t0 = time.perf_counter()
    m, prof, win, meta, tens = _start(case, trained_blob, tmp_path)
    t1 = time.perf_counter()
    try:
        bad, _ = _check_layers(tag, m, prof, win, meta, tens)
        bad += _check_feat_borders(tag, m)
        if stages:
            T = {}
            for s in (1, 2, 3):
                for n in ("feat%d", "volume%d", "s%d.conv11", "logits%d", "depth%d", "conf%d"):
                    T[n % s] = m.tensor(n % s)
            bad += _check_stages(tag, T, win, meta, tens, V)
    finally:
        m.close()
    print("%s wall time: %.2f s engine (upload, forward, profile), %.2f s downloads + float64 references" % (tag, t1 - t0, time.perf_counter() - t1))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", SMALL_CASES + FORCED_CASES + ORDINARY_CASES, ids=[c[0] for c in SMALL_CASES + FORCED_CASES + ORDINARY_CASES])
def test_engine_layers_against_float64(case, trained_blob, tmp_path, monkeypatch):
    """One window per case: every FeatureNet / CostRegNet layer of the engine's plan against the float64 restatement of that layer, the borders of
    feat1..3, and the stage tensors (feat / volume / logits / depth / conf) through test_mvs_stages_gpu._check_stages."""
    _run_case(case, trained_blob, tmp_path, monkeypatch, stages=True)


@pytest.mark.parametrize("case", TUNED_CASES, ids=[c[0] for c in TUNED_CASES])
def test_tuned_shape_layers_against_float64(case, trained_blob, tmp_path, monkeypatch):
    """The two shapes conv_tuned.h holds measured plans for, with its rows applied and with DR_CONV_NO_TUNED=1 (the cost model's own choice): every layer
    of both plans against float64.  (The stage tensors are left to test_mvs_stages_gpu.py: a float64 cost volume of this size takes minutes.)"""
    _run_case(case, trained_blob, tmp_path, monkeypatch, stages=False)


@pytest.mark.parametrize("shape", sorted(TUNED_SHAPES))
def test_tuned_rows_are_applied(shape, trained_blob, tmp_path, monkeypatch):
    """The layers whose kernel differs between the default plan and DR_CONV_NO_TUNED=1 are rows of conv_tuned.h that are really applied at that shape (the
    kernel string shows the family and <ci, ct, pt>; a row that changes the tile shape alone does not show and is not counted).  Not empty at either shape:
    the layer test above really ran tuned plans."""
    with_rows, without = [_profile_of(c, trained_blob, tmp_path, monkeypatch) for c in TUNED_CASES if c[0].startswith("tuned-%s-" % shape)]
    assert with_rows.keys() == without.keys()
    applied = [(op, without[op], k) for op, k in with_rows.items() if _is_layer_op(op) and k != without[op]]
    print()
    for op, a, b in applied:
        print("tuned-%s applied row: %-11s %s -> %s" % (shape, op, a, b))
    print("tuned-%s: %d layers run a tuned plan the kernel string shows" % (shape, len(applied)))
    assert applied, shape


def test_small_windows_run_every_family_of_the_tuned_plans(trained_blob, tmp_path, monkeypatch):
    """The kernel family of a layer op is its kernel string up to `<`.  The union over the small cases (plain and forced) must contain the union over the
    default plans of the two tuned shapes: whatever family the benchmark's plans run has also met a 32-pixel window inside the engine."""
    def union(cases):
        fam = {}
        for c in cases:
            for op, k in _profile_of(c, trained_blob, tmp_path, monkeypatch).items():
                if _is_layer_op(op):
                    fam.setdefault(family(k), []).append("%s:%s" % (c[0], op))
        return fam
    small, tuned = union(SMALL_CASES + FORCED_CASES), union([c for c in TUNED_CASES if not c[6]])
    print()
    for name, fam in (("small", small), ("tuned", tuned)):
        for f in sorted(fam):
            print("families %-5s %-11s %3d ops, e.g. %s" % (name, f, len(fam[f]), fam[f][0]))
    missing = set(tuned) - set(small) - set(REFUSED_AT_SMALL_SHAPES)
    assert not missing, "families of the tuned plans that no small case runs: %s" % sorted(missing)
    assert not set(REFUSED_AT_SMALL_SHAPES) & set(small), "listed as refused at small shapes, yet a small case runs it"
