"""-m gpu: every stage of the depth pipeline between FeatureNet and the edge filter against a float64 restatement of that ONE operation
(tests/mvs_stage_ref.py), fed the engine's own stage input and compared per element -- as test_edge_filter_is_exact_given_the_same_depth does
for the filter.  The A/B tests of tests/test_mvsnet_gpu.py compare kernel generations that share cv_project_ray, cv_warp, make_planes,
plane_depth, regress_regs and prob2_body: a mistake in a shared helper is the same on both sides; the end-to-end bounds let a few border
pixels move by a millimetre.  Here:

  feat_s              against features64(images)                              4 E_FEAT[s] of range      (k_fn_front, k_fn_head3, the u8 preprocessing)
  volume_s            against cost_volume64(feat_s, planes64(depth_{s-1}))    4 E_VOL[s] of range, mean 4 E_VOL_MEAN[s]; the four borders named
  logits_s            against prob64(s{S}.conv11)                             2e-5 of range             (k_prob2 / k_prob2_regress, every z chunking)
  depth_s, conf_s     against regress64(logits_s, planes64(depth_{s-1}))      4 E_DEPTH relative, 4 E_CONF absolute; no pixel excluded

E_* = the fp32 oracle's own error against the same restatements (measured by tests/test_mvs_stage_ref.py, recorded in mvs_stage_ref.py); the
factor 4 is argued there.  Shapes: the smallest that give partial pixel blocks of k_costvol5 at every stage (stage widths 24/48/96, 40/80/160,
16/32/64 against 32 / 64 / 128 pixels per block) and partial and exact 64-column tiles of k_prob2; 2, 4 and 8 views; four pose / range settings
(mvs_stage_ref.make_case), among them samples behind a source camera and a quarter of the samples outside the source images.
Measured on an MI355X (DESIGN.md section 4 has the table): every kernel inside its bound, the largest share of a bound 0.39 (volume2 max)."""
import numpy as np
import pytest

import mvs_stage_ref as R

pytestmark = pytest.mark.gpu

# id, H, W, views, pose, model, DR_PROB_ZCHUNK
CASES = [
    ("trained-64x96-v4-scene", 64, 96, 4, "scene", "trained", None),
    ("trained-96x160-v8-scene-z8", 96, 160, 8, "scene", "trained", 8),
    ("trained-96x64-v2-narrow-z3", 96, 64, 2, "narrow", "trained", 3),
    ("trained-64x96-v4-behind-z5", 64, 96, 4, "behind", "trained", 5),
    ("trained-96x160-v4-rotated", 96, 160, 4, "rotated", "trained", None),
    ("trained-96x64-v8-behind-z8", 96, 64, 8, "behind", "trained", 8),
    ("d4-96x64-v4-behind", 96, 64, 4, "behind", (48, 4, 4), None),
    ("d4-64x96-v2-rotated-z3", 64, 96, 2, "rotated", (48, 4, 4), 3),
    ("generic-64x96-v2-rotated-z8", 64, 96, 2, "rotated", (16, 8, 8), 8),
    ("generic-96x160-v4-scene-z5", 96, 160, 4, "scene", (16, 8, 8), 5),
    ("plain-64x96-v4-narrow", 64, 96, 4, "narrow", "plain", None),
    ("plain-96x64-v8-rotated-z8", 96, 64, 8, "rotated", "plain", 8),
    ("plain-96x160-v2-behind-z3", 96, 160, 2, "behind", "plain", 3),
]


def _model(model, trained_blob, tmp_path):
    """(blob path, meta, tensors): the trained blob; the same tensors with other plane counts; a plain-variance blob of random weights."""
    from tandem_amd import weights as Wt
    if model == "trained":
        meta, tens = Wt.read_blob(trained_blob)
        return trained_blob, meta, tens
    p = str(tmp_path / "w.tdmw")
    if model == "plain":
        Wt.write_blob(p, Wt.random_state((48, 32, 8), seed=11), depth_num=(48, 32, 8), view_aggregation=False)
    else:
        _, tens = Wt.read_blob(trained_blob)
        Wt.write_blob(p, tens, depth_num=model)
    meta, tens = Wt.read_blob(p)
    return p, meta, tens


def _run(blob, win, H, W, V):
    """upload, forward(1), every stage tensor in its logical layout, and the kernels the forward ran."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    m = DrMvsnet(blob)
    m.upload(H, W, V, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), win["depth_min"], win["depth_max"], 2.5)
    m.forward(1)
    T = {}
    for s in (1, 2, 3):
        for n in ("feat%d", "volume%d", "s%d.conv11", "logits%d", "depth%d", "conf%d"):
            T[n % s] = m.tensor(n % s).copy()
    kern = {r["op"]: r["kernel"] for r in m.profile()}
    m.close()
    return T, kern


def _check_stages(tag, T, win, meta, tens, V, features=True):
    """Every stage tensor against its float64 restatement; prints each figure, returns the list of violated bounds."""
    bad = []

    def hold(what, value, bound):
        print("%s %-28s %.3e  (bound %.3e, %.2f of it)" % (tag, what, value, bound, value / bound))
        if not value <= bound:  # (NaN fails)
            bad.append("%s: %.3e > %.3e" % (what, value, bound))

    va = meta["view_aggregation"]
    e_vol, e_mean = (R.E_VOL, R.E_VOL_MEAN) if va else (R.E_VOL_PLAIN, R.E_VOL_PLAIN_MEAN)
    order = R.model_order(V, win["ref_index"])
    c2w = np.stack([np.asarray(win["c2ws"][i], np.float32) for i in order])
    if features:
        f64 = R.features64(win["bgrs"], tens, win["ref_index"])
        for s in (1, 2, 3):
            hold("feat%d max" % s, np.abs(T["feat%d" % s] - f64[s - 1]).max() / R.rng_of(f64[s - 1]), R.BOUND_FACTOR * R.E_FEAT[s])
    prev = None
    for s in (1, 2, 3):
        vol, logits = T["volume%d" % s], T["logits%d" % s][..., 0]
        depth, conf = T["depth%d" % s][0, :, :, 0], T["conf%d" % s][0, :, :, 0]
        D, h, w, _ = vol.shape
        planes = R.planes64(s, prev, win["depth_min"], win["depth_max"], meta, h, w)
        # -- cost volume
        v64, stats = R.cost_volume64(T["feat%d" % s], planes, R.stage_K(win["K"], s), c2w, R.gate_weights(tens, s), va, return_stats=True)
        err, rng = np.abs(vol - v64), R.rng_of(v64)
        print("%s stage %d: %.3f of the samples behind a camera, %.3f outside the image" % (tag, s, stats["behind"], stats["outside"]))
        hold("volume%d max" % s, err.max() / rng, R.BOUND_FACTOR * e_vol[s])
        hold("volume%d mean" % s, err.mean() / rng, R.BOUND_FACTOR * e_mean[s])
        for name, sl in R.border_slices():
            hold("volume%d %s max" % (s, name), err[sl].max() / rng, R.BOUND_FACTOR * e_vol[s])
        # -- prob head
        l64 = R.prob64(T["s%d.conv11" % s], tens["cost_regularization_net.stage%d.prob.weight" % s])
        hold("logits%d max" % s, np.abs(logits - l64).max() / R.rng_of(l64), R.CONV_BOUND)
        # -- regression
        d64, ek, sum4 = R.regress64(logits, planes)
        hold("depth%d max rel" % s, (np.abs(depth - d64) / np.abs(d64)).max(), R.BOUND_FACTOR * R.E_DEPTH)
        cerr, near = R.conf_error(conf, ek, sum4)
        hold("conf%d max (%d px near an integer E[k])" % (s, int(near.sum())), cerr.max(), R.BOUND_FACTOR * R.E_CONF)
        prev = depth
    return bad


def _expected_kernels(meta, zchunk, dchunk=None):
    want = {}
    for s in (1, 2, 3):
        D, C = meta["depth_num"][s - 1], 32 >> (s - 1)
        if meta["view_aggregation"]:
            want["s%d.costvol" % s] = "k_costvol5<%d,%d>" % (C, min(D, dchunk) if dchunk else 4)
        else:
            want["s%d.costvol" % s] = "k_costvol3<%d>" % C
        # (small frames: the default z chunk is 2; a D = 8 stage in one chunk runs prob and regression in one launch)
        want["s%d.prob" % s] = "k_prob2_regress<8>" if D == 8 and zchunk is not None and zchunk >= 8 else "k_prob2<1>"
    return want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stage_tensors_against_float64(case, trained_blob, tmp_path, monkeypatch):
    """One window per case: feat / volume / logits / depth / conf of all three stages against the float64 restatements, each fed the engine's own
    stage input.  Models: the trained blob (48/32/8: k_costvol5, k_regress_r<48/32/8>, with DR_PROB_ZCHUNK=8 k_prob2_regress<8>), the same tensors
    at 48/4/4 (the D = 4 paths) and 16/8/8 (stage 1: the generic k_regress), a plain-variance blob (k_costvol3).  DR_PROB_ZCHUNK unset, 3, 5, 8:
    z chunks that do and do not divide D.  The regression kernel follows from the plane count alone (48, 32, 8, 4: k_regress_r<D>), the profile
    names the other two."""
    tag, H, W, V, pose, model, zchunk = case
    if zchunk is None:
        monkeypatch.delenv("DR_PROB_ZCHUNK", raising=False)
    else:
        monkeypatch.setenv("DR_PROB_ZCHUNK", str(zchunk))
    for s in (1, 2, 3):
        monkeypatch.delenv("DR_CV_DCHUNK%d" % s, raising=False)
    blob, meta, tens = _model(model, trained_blob, tmp_path)
    win = R.make_case(H, W, V, pose)
    T, kern = _run(blob, win, H, W, V)
    for op, k in _expected_kernels(meta, zchunk).items():
        assert kern.get(op) == k, (op, kern.get(op), k)
    bad = _check_stages(tag, T, win, meta, tens, V)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("library", ["product", "parity"])
def test_stage_tensors_with_depth_chunks_of_eight(library, trained_blob, tmp_path, monkeypatch, request):
    """DR_CV_DCHUNK{1,2,3}=8: k_costvol5's eight-plane chunk (the product's is four), in the product library and once in the parity build."""
    if library == "parity":
        request.getfixturevalue("parity_hooks")
    monkeypatch.delenv("DR_PROB_ZCHUNK", raising=False)
    for s in (1, 2, 3):
        monkeypatch.setenv("DR_CV_DCHUNK%d" % s, "8")
    blob, meta, tens = _model("trained", trained_blob, tmp_path)
    win = R.make_case(64, 96, 4, "behind")
    T, kern = _run(blob, win, 64, 96, 4)
    for op, k in _expected_kernels(meta, None, dchunk=8).items():
        assert kern.get(op) == k, (op, kern.get(op), k)
    bad = _check_stages("dchunk8-" + library, T, win, meta, tens, 4, features=False)
    assert not bad, "\n".join(bad)
