"""CPU: the float64 stage restatements of tests/mvs_stage_ref.py against the fp32 oracle (oracle/mvsnet_oracle.py), stage by stage on
the oracle's own stage inputs.  Two things come out of it:

 * the restatements are validated against the oracle's grid_sample / ATen formulation, and the oracle's own fp32 rounding error per
   stage is MEASURED: the E_* constants recorded in mvs_stage_ref.py, which the GPU test's bounds are multiples of.  The oracle must
   stay within 1.5 x the recorded figures, so drift is noticed;
 * every listed one-line mistake (mvs_stage_ref.MUTANTS) moves the float64 cost volume by more than the bound the GPU test sets, at some
   stage of some window: the windows are not too tame for the bound to separate rounding from a wrong kernel.  The behind-camera mask
   (pz < 0.001) in particular needs a source camera AHEAD of the reference by more than depth_min: the scene's own poses never put a
   sample there that would otherwise be read.
"""
import os

import numpy as np
import pytest
import torch

import mvs_stage_ref as R

_CACHE = {}


def _window(spec, trained_blob, plain=False, model="trained"):
    """Oracle forward with its stage tensors + the float64 base volumes of one window, computed once per session.
    model: "trained", "plain" (= plain=True) or a plane-count triple (the trained tensors with other plane counts)."""
    model = "plain" if plain else model
    key = (spec, model)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import mvsnet_oracle as O
    from tandem_amd import weights as Wt
    if model == "plain":
        tens = Wt.random_state((48, 32, 8), seed=11)
        meta = dict(depth_num=(48, 32, 8), interval_ratio=(1.0, 0.5, 0.25), view_aggregation=False, base_channels=8)
    else:
        meta, tens = Wt.read_blob(trained_blob)
        if model != "trained":
            meta = dict(meta, depth_num=tuple(model))
    H, W, V, pose = spec
    win = R.make_case(H, W, V, pose)
    out = O.forward(O.Weights(meta, tens), win["bgrs"], win["K"], win["c2ws"], win["ref_index"], win["depth_min"], win["depth_max"], 2.5,
                    return_debug=True)
    order = R.model_order(V, win["ref_index"])
    c2w = np.stack([np.asarray(win["c2ws"][i], np.float32) for i in order])
    st = {}
    for s in (1, 2, 3):
        dbg = out["debug"][s]
        feats = out["debug"]["features"][s - 1].permute(0, 2, 3, 1).double().numpy()   # (V, h, w, C)
        planes = dbg["planes"].double().numpy()
        args = (feats, planes, R.stage_K(win["K"], s), c2w, R.gate_weights(tens, s), meta["view_aggregation"])
        vol64, stats = R.cost_volume64(*args, return_stats=True)
        st[s] = dict(args=args, vol64=vol64, stats=stats, vol32=dbg["volume"].permute(1, 2, 3, 0).numpy(), planes=planes,
                     logits=dbg["logits"].numpy(), depth=out["stages"][s]["depth_dense"].numpy(), conf=out["stages"][s]["confidence_dense"].numpy())
    res = dict(win=win, meta=meta, tens=tens, out=out, st=st)
    _CACHE[key] = res
    return res


PLAIN_WINDOWS = ((64, 96, 4, "narrow"), (96, 64, 3, "rotated"), (96, 160, 2, "behind"))
SMALL = tuple(zip(R.SMALL_WINDOWS, R.SMALL_MODELS))
LAYER_WINDOWS = tuple((spec, "trained") for spec in R.CPU_WINDOWS) + SMALL  # what E_LAYER is the maximum over


def _oracle_tensors(w):
    """Every tensor mvs_stage_ref.all_layers() names, from the fp32 oracle, in the engine's layouts: FeatureNet layer by layer through the oracle's own
    layer function (the chain is checked to BE the oracle's feature_net, bit for bit), CostRegNet through cost_reg(return_all=True)."""
    if "oracle_tensors" in w:
        return w["oracle_tensors"]
    import torch.nn.functional as F
    from oracle import mvsnet_oracle as O
    win, ow, p = w["win"], O.Weights(w["meta"], w["tens"]), "feature_net."
    T = {}
    with torch.no_grad():
        image, _, _ = O.preprocess(win["bgrs"], win["K"], win["c2ws"], win["ref_index"])
        x = O._cbr2(O._cbr2(image, ow, p + "conv0.0", 1, 1), ow, p + "conv0.1", 1, 1)
        T["fn.conv0.1"] = x
        for blk in (1, 2):
            for i, (stride, pad) in enumerate(((2, 2), (1, 1), (1, 1))):
                x = O._cbr2(x, ow, p + "conv%d.%d" % (blk, i), stride, pad)
                T["fn.conv%d.%d" % (blk, i)] = x
        c3, c2, c1 = T["fn.conv0.1"], T["fn.conv1.2"], T["fn.conv2.2"]
        T["feat1"] = F.conv2d(c1, ow[p + "out.stage1.weight"])
        T["inter2"] = F.interpolate(c1, scale_factor=2, mode="nearest") + F.conv2d(c2, ow[p + "skip.stage2.weight"], ow[p + "skip.stage2.bias"])
        T["feat2"] = F.conv2d(T["inter2"], ow[p + "out.stage2.weight"], None, 1, 1)
        i3 = F.interpolate(T["inter2"], scale_factor=2, mode="nearest") + F.conv2d(c3, ow[p + "skip.stage3.weight"], ow[p + "skip.stage3.bias"])
        T["feat3"] = F.conv2d(i3, ow[p + "out.stage3.weight"], None, 1, 1)
        for s in (1, 2, 3):
            assert torch.equal(T["feat%d" % s], w["out"]["debug"]["features"][s - 1]), s
        T = {k: v.permute(0, 2, 3, 1).numpy() for k, v in T.items()}
        assert np.array_equal(image.permute(0, 2, 3, 1).numpy(), R.image64(win["bgrs"], win["ref_index"]))  # the u8 -> float image, exactly
        for s in (1, 2, 3):
            vol = w["out"]["debug"][s]["volume"]
            logits, mid = O.cost_reg(vol, ow, s, return_all=True)
            assert torch.equal(logits, w["out"]["debug"][s]["logits"]), s
            T["volume%d" % s] = vol.permute(1, 2, 3, 0).numpy()
            for k, v in mid.items():
                T["s%d.conv%s" % (s, k[1:])] = v.permute(1, 2, 3, 0).numpy()
    w["oracle_tensors"] = T
    return T


def _layer_inputs(layer, T, win):
    return [R.image64(win["bgrs"], win["ref_index"]) if n == "images" else T[n] for n in layer.inputs]


def _layer_errors(w):
    """{engine tensor: (error as a share of layer_scale, as a share of the output's range)} of the fp32 oracle's layer against the float64 restatement
    given the oracle's own input."""
    if "layer_errors" not in w:
        T, res = _oracle_tensors(w), {}
        for layer in R.all_layers(w["meta"]):
            out, pre = layer.fn(*_layer_inputs(layer, T, w["win"]), w["tens"])
            assert out.shape == T[layer.name].shape, (layer.name, out.shape, T[layer.name].shape)
            err = float(np.abs(T[layer.name] - out).max())
            res[layer.name] = (err / R.layer_scale(out, pre), err / max(R.rng_of(out), 1e-300))
        w["layer_errors"] = res
    return w["layer_errors"]


def test_reference_error_is_measured_and_has_not_drifted(trained_blob):
    """The fp32 oracle against the float64 restatement per stage, given the oracle's own inputs; prints the E_* block of mvs_stage_ref.py."""
    e_vol, e_mean, e_feat = {1: 0.0, 2: 0.0, 3: 0.0}, {1: 0.0, 2: 0.0, 3: 0.0}, {1: 0.0, 2: 0.0, 3: 0.0}
    p_vol, p_mean = {1: 0.0, 2: 0.0, 3: 0.0}, {1: 0.0, 2: 0.0, 3: 0.0}
    e_depth = e_conf = 0.0
    for plain, specs in ((False, R.CPU_WINDOWS), (True, PLAIN_WINDOWS)):
        for spec in specs:
            w = _window(spec, trained_blob, plain)
            win, meta = w["win"], w["meta"]
            f64 = R.features64(win["bgrs"], w["tens"], win["ref_index"])
            prev = None
            for s in (1, 2, 3):
                t = w["st"][s]
                err = np.abs(t["vol32"] - t["vol64"]) / R.rng_of(t["vol64"])
                (p_vol if plain else e_vol)[s] = max((p_vol if plain else e_vol)[s], float(err.max()))
                (p_mean if plain else e_mean)[s] = max((p_mean if plain else e_mean)[s], float(err.mean()))
                # the planes: each is a handful of fp32 operations on values <= the largest plane, 2^-24 of it apiece
                h, w_ = t["planes"].shape[1:]
                p64 = R.planes64(s, prev, win["depth_min"], win["depth_max"], meta, h, w_)
                assert np.abs(p64 - t["planes"]).max() <= 2e-6 * np.abs(p64).max(), (spec, s)
                prev = t["depth"]
                f32 = w["out"]["debug"]["features"][s - 1].permute(0, 2, 3, 1).numpy()
                e_feat[s] = max(e_feat[s], float(np.abs(f32 - f64[s - 1]).max() / R.rng_of(f64[s - 1])))
                depth, ek, sum4 = R.regress64(t["logits"], t["planes"])
                e_depth = max(e_depth, float((np.abs(t["depth"] - depth) / np.abs(depth)).max()))
                cerr, _ = R.conf_error(t["conf"], ek, sum4)
                e_conf = max(e_conf, float(cerr.max()))
    # one layer at a time (mvs_stage_ref "THE LAYER RESTATEMENTS"): CPU_WINDOWS and the smallest windows, every CostRegNet and FeatureNet layer
    e_layer, where = 0.0, None
    for spec, model in LAYER_WINDOWS:
        for name, (err, _) in _layer_errors(_window(spec, trained_blob, model=model)).items():
            if err > e_layer:
                e_layer, where = err, (spec, model, name)
    fmt = lambda d: "{" + ", ".join("%d: %.2e" % (k, v) for k, v in d.items()) + "}"  # noqa: E731
    print("\nE_VOL = %s\nE_VOL_MEAN = %s\nE_VOL_PLAIN = %s\nE_VOL_PLAIN_MEAN = %s\nE_DEPTH = %.2e\nE_CONF = %.2e\nE_FEAT = %s\nE_LAYER = %.2e"
          % (fmt(e_vol), fmt(e_mean), fmt(p_vol), fmt(p_mean), e_depth, e_conf, fmt(e_feat), e_layer))
    print("(E_LAYER at %s; CONV_BOUND / E_LAYER = %.1f)" % (where, R.CONV_BOUND / e_layer))
    assert e_layer <= 1.5 * R.E_LAYER, (e_layer, where)
    assert R.BOUND_FACTOR * R.E_LAYER <= R.CONV_BOUND  # the layer bound of the GPU test is a margin over the reference's own error, not a fit
    for s in (1, 2, 3):
        assert e_vol[s] <= 1.5 * R.E_VOL[s] and e_mean[s] <= 1.5 * R.E_VOL_MEAN[s], (s, e_vol[s], e_mean[s])
        assert p_vol[s] <= 1.5 * R.E_VOL_PLAIN[s] and p_mean[s] <= 1.5 * R.E_VOL_PLAIN_MEAN[s], (s, p_vol[s], p_mean[s])
        assert e_feat[s] <= 1.5 * R.E_FEAT[s], (s, e_feat[s])
    assert e_depth <= 1.5 * R.E_DEPTH and e_conf <= 1.5 * R.E_CONF, (e_depth, e_conf)


def test_prob64_is_the_oracles_prob_head(trained_blob):
    """prob64 on the oracle's x11 against the oracle's logits: the same conv3d, held to the project's convolution bound."""
    from oracle import mvsnet_oracle as O
    w = _window(R.CPU_WINDOWS[0], trained_blob)
    ow = O.Weights(w["meta"], w["tens"])
    for s in (1, 2, 3):
        with torch.no_grad():
            logits, mid = O.cost_reg(w["out"]["debug"][s]["volume"], ow, s, return_all=True)
        l64 = R.prob64(mid["x11"].permute(1, 2, 3, 0).numpy(), w["tens"]["cost_regularization_net.stage%d.prob.weight" % s])
        assert np.abs(logits.numpy() - l64).max() <= R.CONV_BOUND * R.rng_of(l64), s


def test_the_windows_reach_the_masks(trained_blob):
    """The `behind` window puts samples behind a source camera (a non-zero share, at every stage), the `rotated` one sends about a quarter of
    its samples out of the source images; the scene's own poses do neither to a sample behind the camera."""
    behind = _window((64, 96, 4, "behind"), trained_blob)
    for s in (1, 2, 3):  # ... and the mask decides there: without it the volume moves beyond the GPU test's bound at EVERY stage
        t = behind["st"][s]
        assert t["stats"]["behind"] > 0.0, s
        moved = np.abs(R.cost_volume64(*t["args"], mutant="no_behind_mask") - t["vol64"]).max() / R.rng_of(t["vol64"])
        assert moved > 20.0 * R.BOUND_FACTOR * R.E_VOL[s], (s, moved)
    rotated = _window((64, 96, 3, "rotated"), trained_blob)
    for s in (1, 2, 3):
        assert 0.15 < rotated["st"][s]["stats"]["outside"] < 0.45, (s, rotated["st"][s]["stats"])
    print("\nbehind shares", [behind["st"][s]["stats"]["behind"] for s in (1, 2, 3)], "outside shares (rotated)", [rotated["st"][s]["stats"]["outside"] for s in (1, 2, 3)])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_moves_the_volume_beyond_the_gpu_bound(trained_blob, mutant):
    """max |volume(mutant) - volume| must exceed BOUND_FACTOR * E_VOL[s] * range -- the bound tests/test_mvs_stages_gpu.py holds the kernels to --
    at some stage of at least one window (and be told apart by a wide margin: a factor 20 at least)."""
    best, where = 0.0, None
    for spec in R.CPU_WINDOWS:
        if mutant == "no_behind_mask" and spec[3] != "behind":
            continue  # (checked below: it changes nothing elsewhere)
        w = _window(spec, trained_blob)
        for s in (2, 3) if mutant == "spacing_Dm1" else (1, 2, 3):
            t = w["st"][s]
            moved = np.abs(R.cost_volume64(*t["args"], mutant=mutant) - t["vol64"]).max() / R.rng_of(t["vol64"])
            ratio = moved / (R.BOUND_FACTOR * R.E_VOL[s])
            if ratio > best:
                best, where = ratio, (spec, s, moved)
    print("\n%s: %.1f x the GPU bound at %s" % (mutant, best, where))
    assert best > 20.0, (mutant, best, where)


def test_the_scene_poses_never_needed_the_behind_camera_mask(trained_blob):
    """With the scene's own poses the mask is dead code even at 0.01 .. 10: removing it changes no voxel."""
    from oracle import mvsnet_oracle as O
    from synth import scene
    from tandem_amd import weights as Wt
    meta, tens = Wt.read_blob(trained_blob)
    win = scene.make_window(64, 96, 7, seed=17)
    out = O.forward(O.Weights(meta, tens), win["bgrs"], win["K"], win["c2ws"], win["ref_index"], 0.01, 10.0, 2.5, return_debug=True)
    order = R.model_order(7, win["ref_index"])
    c2w = np.stack([np.asarray(win["c2ws"][i], np.float32) for i in order])
    for s in (1, 2, 3):
        feats = out["debug"]["features"][s - 1].permute(0, 2, 3, 1).double().numpy()
        args = (feats, out["debug"][s]["planes"].double().numpy(), R.stage_K(win["K"], s), c2w, R.gate_weights(tens, s), True)
        a, stats = R.cost_volume64(*args, return_stats=True)
        b = R.cost_volume64(*args, mutant="no_behind_mask")
        print("\nstage %d: behind share %.3e" % (s, stats["behind"]))
        assert np.array_equal(a, b), s


def test_reference_error_holds_at_the_smallest_windows(trained_blob):
    """The recorded E_* figures (maxima over CPU_WINDOWS, unchanged) also hold, within the same 1.5 x, at the smallest windows the engine accepts --
    32-pixel sides, stage-1 maps of 8 x 8 -- with the 48/32/8, 48/4/4 and 16/8/8 plane counts: the GPU test's factor 4 needs no change there."""
    worst = {}

    def hold(what, value, recorded, spec):
        r = value / recorded
        if r > worst.get(what, (0.0, None))[0]:
            worst[what] = (r, spec)

    for spec, model in SMALL:
        w = _window(spec, trained_blob, model=model)
        win, meta = w["win"], w["meta"]
        assert all(np.isfinite(w["out"][k]).all() for k in ("depth", "confidence", "depth_dense", "confidence_dense")), spec
        f64 = R.features64(win["bgrs"], w["tens"], win["ref_index"])
        prev = None
        for s in (1, 2, 3):
            t = w["st"][s]
            err = np.abs(t["vol32"] - t["vol64"]) / R.rng_of(t["vol64"])
            hold("E_VOL[%d]" % s, float(err.max()), R.E_VOL[s], spec)
            hold("E_VOL_MEAN[%d]" % s, float(err.mean()), R.E_VOL_MEAN[s], spec)
            h, w_ = t["planes"].shape[1:]
            p64 = R.planes64(s, prev, win["depth_min"], win["depth_max"], meta, h, w_)
            assert np.abs(p64 - t["planes"]).max() <= 2e-6 * np.abs(p64).max(), (spec, s)
            prev = t["depth"]
            f32 = w["out"]["debug"]["features"][s - 1].permute(0, 2, 3, 1).numpy()
            hold("E_FEAT[%d]" % s, float(np.abs(f32 - f64[s - 1]).max() / R.rng_of(f64[s - 1])), R.E_FEAT[s], spec)
            depth, ek, sum4 = R.regress64(t["logits"], t["planes"])
            hold("E_DEPTH", float((np.abs(t["depth"] - depth) / np.abs(depth)).max()), R.E_DEPTH, spec)
            cerr, _ = R.conf_error(t["conf"], ek, sum4)
            hold("E_CONF", float(cerr.max()), R.E_CONF, spec)
    print()
    for what, (r, spec) in sorted(worst.items()):
        print("small windows: %-14s %.2f x the recorded figure at %s" % (what, r, spec))
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.5}
    assert not bad, bad


@pytest.mark.parametrize("mutant", R.LAYER_MUTANTS)
def test_every_layer_mutant_moves_a_small_window_beyond_the_gpu_bound(trained_blob, mutant):
    """Each one-line mistake of a layer moves some layer of some small window by more than 20 x CONV_BOUND of the layer's scale -- the bound
    tests/test_mvs_layers_gpu.py holds the engine's layers to: the small windows are not too tame for it."""
    best, where = 0.0, None
    for spec, model in SMALL:
        w = _window(spec, trained_blob, model=model)
        T = _oracle_tensors(w)
        for layer in R.all_layers(w["meta"]):
            if mutant not in layer.mutants():
                continue
            x = _layer_inputs(layer, T, w["win"])
            out, pre = layer.fn(*x, w["tens"])
            moved = float(np.abs(layer.fn(*x, w["tens"], mutant=mutant)[0] - out).max()) / R.layer_scale(out, pre)
            if moved > best:
                best, where = moved, (spec, model, layer.name)
    print("\n%s: moves a layer by %.3g of its scale = %.0f x the bound, at %s" % (mutant, best, best / R.CONV_BOUND, where))
    assert best > 20.0 * R.CONV_BOUND, (mutant, best, where)
